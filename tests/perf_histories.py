"""Seeded generators of histories for the perf tests (jepsen/perf.py, tbc_perf_series): `Builder` writes ops one by one (the shape cases
lay out cells, bucket edges and classes exactly), `random_history` simulates workers; `shape_cases()` lists the smallest shapes at
which each kernel of csrc/perf_kernels.h can go wrong, `expected` turns the host statement (`perf.analyse`) into the arrays
tbc_perf_series returns, and `references` computes it once per case after asserting that the case has the shape it is named for."""
import random

import numpy as np

from jepsen_tigerbeetle_amd.jepsen import perf as PF

S = 10 ** 9
INT32_MIN, INT64_MIN = -(2 ** 31), -(2 ** 63)
CODE = {None: 0, "ok": 1, "fail": 2, "info": 3}


class Builder:
    def __init__(self):
        self.h = []

    def op(self, type_, f, process, time):
        self.h.append({"type": type_, "f": f, "value": None, "process": process, "time": time})
        return self

    def pair(self, f, process, t0, latency, outcome="ok"):
        return self.op("invoke", f, process, t0).op(outcome, f, process, t0 + latency)

    def nemesis(self, time, f="kill"):
        return self.op("info", f, "nemesis", time)


def random_history(seed, n_ops, workers=5, fs=("read", "write"), gap=30_000_000, info=0.05, fail=0.1, nemesis=0.02, jitter=0):
    """`n_ops` ops of `workers` workers: an idle worker invokes, a busy one completes (ok / fail / info); after an :info the worker takes
    a new process number half of the time and keeps its own otherwise; now and then the nemesis speaks.  Times rise by random gaps, with
    `jitter` ns taken off some so that they are not monotone."""
    rng = random.Random(seed)
    h, t = [], 0
    proc = list(range(workers))
    busy = [None] * workers
    while len(h) < n_ops:
        t += rng.randrange(1, 2 * gap)
        when = max(0, t - rng.randrange(jitter)) if jitter and rng.random() < 0.3 else t
        if rng.random() < nemesis:
            h.append({"type": "info", "f": rng.choice(("kill", "heal")), "value": None, "process": "nemesis", "time": when})
            continue
        w = rng.randrange(workers)
        if busy[w] is None:
            busy[w] = rng.choice(fs)
            h.append({"type": "invoke", "f": busy[w], "value": None, "process": proc[w], "time": when})
        else:
            r = rng.random()
            ty = "info" if r < info else ("fail" if r < info + fail else "ok")
            h.append({"type": ty, "f": busy[w], "value": None, "process": proc[w], "time": when})
            busy[w] = None
            if ty == "info" and rng.random() < 0.5:
                proc[w] += workers
    return h


def cells_history(sizes, latency, f="read"):
    """one f, cell k (bucket k) of sizes[k] matched invocations with latencies latency(k, i), each by a process of its own; the
    completions follow all invocations, in another order"""
    b = Builder()
    done = []
    p = 0
    for k, n in enumerate(sizes):
        for i in range(n):
            t0 = k * S + 1000 * i + 7
            b.op("invoke", f, p, t0)
            done.append((p, t0 + latency(k, i)))
            p += 1
    for p, t1 in done[::-1]:
        b.op("ok", f, p, t1)
    return b.h


def tmax_history(t_last):
    """a few client ops in the first three seconds, and a last completion at t_last"""
    b = Builder()
    b.pair("read", 0, 100, 5_000).pair("write", 1, S + 5, S)
    b.op("invoke", "read", 2, 2 * S + S // 2).op("ok", "read", 2, t_last)
    return b.h


def shape_cases():
    """[{"name", "history", "max_cell", and what else the case must show: "n_plot" ("all" / "less"), "fs", ...}]"""
    cases = []

    def add(name, h, max_cell, **kw):
        cases.append(dict(kw, name=name, history=h, n_ops=len(h), max_cell=max_cell))

    # ---- ops
    add("ops_0", [], 0)
    add("ops_1_lone_invocation", Builder().op("invoke", "read", 0, 5).h, 0)
    add("ops_2", Builder().pair("read", 0, 5, 1000).h, 1)
    for n in (63, 64, 65, 255, 256, 257, 513):
        add(f"ops_{n}", random_history(n, n), None)
    # ---- cell sizes of the select
    sizes = (1, 2, 3, 20, 64, 65, 100, 101)
    add("cells_1_to_101", cells_history(sizes, lambda k, i: (i * 7919 + k) % 1000 * 1000 + 9 * S), 101, cells=sizes)
    add("cell_over_the_tile", cells_history((PF.N.PERF_SELECT_TILE + 52,), lambda k, i: (i * 104729) % 9973 * 100_000 + 3 * S), PF.N.PERF_SELECT_TILE + 52)
    add("cell_of_ties", cells_history((70, 5), lambda k, i: 123_456 + 2 * S), 70)
    add("cell_latency_0", cells_history((5, 40), lambda k, i: 0 if (k == 0 or i % 3 == 0) else 2 * S + i), 40, zero_latency=True)
    add("cell_over_2_32_beside_small", cells_history((40, 3), lambda k, i: (5 * S + i * (2 ** 33)) if i % 2 else 10 + i), 40, wide=True)
    add("cells_every_n_1_to_130", cells_history(tuple(range(1, 131)), lambda k, i: ((i * 31 + k * 17) % 257) * 1_000_003 + 131 * S), 130,
        cells=tuple(range(1, 131)))
    # ---- times
    for tag, t_last, n_plot in (("k_minus_1", 3 * S - 1, "all"), ("k", 3 * S, "less"), ("mid_minus_1", 3 * S + S // 2 - 1, "less"),
                                ("mid", 3 * S + S // 2, "all"), ("mid_plus_1", 3 * S + S // 2 + 1, "all")):
        add(f"tmax_{tag}", tmax_history(t_last), 1, n_plot=n_plot)
    b = Builder()
    edges = [k * S + d for k in (1, 2) for d in (-1, 0, S // 2 - 1, S // 2, S // 2 + 1)]
    for p, t in enumerate(edges):
        b.op("invoke", "read", p, t)
    for p, t in enumerate(edges):
        b.op("ok" if p % 2 else "fail", "read", p, edges[(p + 3) % len(edges)] + 4 * S)
    add("op_times_on_the_edges", b.h, 5)
    add("pair_across_buckets", Builder().pair("read", 0, S - 5, 10).pair("read", 1, 2 * S - 1, 3 * S).h, 1)
    add("empty_buckets_between", Builder().op("invoke", "read", 0, S // 5).op("invoke", "read", 1, S // 4).op("ok", "read", 0, 40 * S + 3 * S // 10)
        .op("ok", "read", 1, 41 * S + 9 * S // 10).h, 2, n_plot="all")
    add("ops_in_the_unplotted_bucket", Builder().pair("read", 0, 10, 20).pair("read", 1, 5 * S + 10, 1000).pair("write", 2, 5 * S + 20, S // 10).h, 1,
        n_plot="less")
    add("times_not_monotone", random_history(7, 200, jitter=2 * S, gap=60_000_000), None, negative_latency=True)
    add("tmax_by_the_nemesis", Builder().pair("read", 0, 10, S).pair("read", 1, 2 * S, S // 2).nemesis(9 * S + 7 * S // 10).h, 1, nemesis_tmax=True)
    # ---- classes
    add("one_f", random_history(11, 120, fs=("read",)), None, fs=1)
    add("nine_fs", random_history(12, 400, workers=9, fs=tuple(f"f{i}" for i in range(9))), None, fs=9)
    b = Builder().pair("read", 0, 10, 100)
    for i in range(5):
        b.pair("cas", 1, 1000 * (i + 1), 500 + i, "fail")
    add("f_with_only_fail", b.h, 5, only={"cas": "fail"})
    b = Builder().pair("read", 0, 10, 100)
    for i in range(4):
        b.op("invoke", "stuck", 10 + i, 2000 + i)
    add("f_with_only_unmatched", b.pair("read", 0, S, 100).h, 1, no_series="stuck")
    add("info_completions", random_history(13, 150, info=0.5, fail=0.0), None, info=True)
    add("process_reused_after_info", Builder().op("invoke", "write", 3, 10).op("info", "write", 3, 500).op("invoke", "write", 3, 900)
        .op("ok", "write", 3, 1500).op("invoke", "write", 3, 2000).op("invoke", "write", 3, 2500).op("ok", "write", 3, S + 1).h, 3)
    add("completion_without_invocation", Builder().op("ok", "read", 0, 10).pair("read", 0, 20, 30).op("fail", "read", 4, S + 1).op("ok", "read", 0, S + 2).h,
        1, orphan=True)
    # ---- the open scan
    b = Builder()
    for i in range(300):
        b.op("invoke", "add", i, 1000 * i)
    for i in range(300):
        b.op("ok", "add", (i * 7) % 300, S + 1000 * i)
    add("open_one_class_over_chunks", b.h, 300, open_peak=300)
    b = Builder()
    for i in range(100):
        b.op("invoke", "a", 2 * i, 1000 * (2 * i)).op("invoke", "b", 2 * i + 1, 1000 * (2 * i + 1))
    for i in range(100):
        b.op("ok", "a", 2 * i, S + 2000 * i).op("fail", "b", 2 * i + 1, S + 2000 * i + 1000)
    add("open_two_classes_interleaved", b.h, 100)
    b = Builder()
    for i in range(160):
        b.pair("read", 0, 4000 * i, 1000)
    add("open_back_to_0_on_the_edge", b.h, 160, zero_at=(63, 127, 255))
    return cases


def expected(history):
    """what tbc_perf_series returns for `history`, from the host statement"""
    a = PF.analyse(history)
    fs, nb, npl = a["fs"], a["nb_all"], a["n_plot"]
    nf = len(fs)
    num = {f: k for k, f in enumerate(fs)}
    n = len(history)
    out = {"op_latency": np.array([INT64_MIN if x is None else x for x in a["latency"]], np.int64).reshape(n),
           "op_outcome": np.array([CODE[x] for x in a["outcome"]], np.uint8).reshape(n),
           "op_open_after": np.array(a["open_after"], np.int32).reshape(n),
           "q_count": np.zeros((nf, nb), np.uint32), "q_value": np.zeros((nf, nb, 4), np.int64), "rate_count": np.zeros((nf, 3, nb), np.uint32),
           "open_last": np.full((nf, 3, nb), INT32_MIN, np.int32), "open_fill": np.zeros((nf, 3, npl), np.int32)}
    for f, cells in a["q_cells"].items():
        for b, lats in cells.items():
            out["q_count"][num[f], b] = len(lats)
            out["q_value"][num[f], b] = [lats[min(len(lats) - 1, int(len(lats) * q))] for q in PF.QS]
    for (f, t), cells in a["rate"].items():
        for b, c in cells.items():
            out["rate_count"][num[f], CODE[t] - 1, b] = c
    for (f, t), cells in a["open_last"].items():
        cur = 0
        for b in range(nb):
            if b in cells:
                out["open_last"][num[f], CODE[t] - 1, b] = cur = cells[b]
            if b < npl:
                out["open_fill"][num[f], CODE[t] - 1, b] = cur
    client = [op for op in history if PF.H.client_op(op)]
    out["summary"] = {"n_ops": n, "n_client": len(client), "n_invocations": sum(op["type"] == "invoke" for op in client),
                      "n_matched": sum(x is not None for x in a["latency"]), "n_completions": sum(op["type"] != "invoke" for op in client),
                      "n_f": nf, "nb_all": nb, "n_plot": npl, "max_cell": int(out["q_count"].max()) if out["q_count"].size else 0, "t_max": a["t_max"]}
    return out


def assert_same(got, want, ctx=""):
    for k, w in want.items():
        if k == "summary":
            g = {f: v for f, v in got[k].items() if f not in ("ns_device", "bytes_in")}
            assert g == w, (ctx, k, g, w)
        else:
            assert got[k].shape == w.shape and got[k].dtype == w.dtype, (ctx, k, got[k].shape, w.shape)
            assert np.array_equal(got[k], w), (ctx, k, np.argwhere(got[k] != w)[:5].tolist())


def references(cases):
    """{name: expected(history)}, each case first shown to have the shape it is named for"""
    refs = {}
    for c in cases:
        h, want = c["history"], expected(c["history"])
        s, a = want["summary"], PF.analyse(h)
        assert s["n_ops"] == c["n_ops"], c["name"]
        if c["max_cell"] is not None:
            assert s["max_cell"] == c["max_cell"], (c["name"], s["max_cell"])
        if "cells" in c:
            assert tuple(int(x) for x in want["q_count"][0])[:len(c["cells"])] == c["cells"], c["name"]
        if "n_plot" in c:
            assert s["n_plot"] == (s["nb_all"] if c["n_plot"] == "all" else s["nb_all"] - 1), c["name"]
        if "fs" in c:
            assert s["n_f"] == c["fs"], c["name"]
        if c.get("zero_latency"):
            assert (want["op_latency"] == 0).sum() >= 5 and (want["q_value"][0, 0] == 0).all()
        if c.get("wide"):
            assert want["q_value"].max() > 2 ** 32 and ((want["op_latency"] >= 0) & (want["op_latency"] < 100)).any()
        if c.get("negative_latency"):
            lat = want["op_latency"]
            assert (lat[lat != INT64_MIN] < 0).any() and any(h[i]["time"] > h[i + 1]["time"] for i in range(len(h) - 1))
        if c.get("nemesis_tmax"):
            assert a["t_max"] > max(op["time"] for op in h if PF.H.client_op(op)) and s["nb_all"] == 10
        if "only" in c:
            (f, t), = c["only"].items()
            assert {k[1] for k in a["rate"] if k[0] == f} == {t}
        if "no_series" in c:
            ser = PF.series_host(h)
            assert c["no_series"] in a["fs"] and not any(k[0] == c["no_series"] for d in ser.values() for k in d)
        if c.get("info"):
            assert (want["op_outcome"] == CODE["info"]).sum() > 20
        if c.get("orphan"):
            assert want["op_open_after"].min() < 0 and s["n_completions"] > s["n_matched"]
        if "open_peak" in c:
            assert want["op_open_after"].max() == c["open_peak"] and c["n_ops"] > 3 * 64 * 3
        if "zero_at" in c:
            assert all(want["op_open_after"][i] == 0 and h[i]["type"] == "ok" for i in c["zero_at"])
        refs[c["name"]] = want
    edge_plots = {c["name"]: refs[c["name"]]["summary"]["n_plot"] - refs[c["name"]]["summary"]["nb_all"] for c in cases if c["name"].startswith("tmax_")}
    assert set(edge_plots.values()) == {0, -1}, edge_plots
    return refs

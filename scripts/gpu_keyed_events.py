"""One keyed history, split by key and paired, into a batch and in one call: the device route against the route that was there, on one
interleaved history of K keys x M ops (synth.register_events per key, 64 processes, 256 distinct histories repeated, their rows
interleaved round-robin, scattered key values).
INTO A BATCH (the batch's event slots are pinned memory; the bench's batch options; every route ends with run()):
  (a) numpy split_events + the rows moved into the split order + Batch.stream_events + run -- what there was
  (b) Batch.stream_keyed_events + run, its pieces (packing into the slot, the submit call, its ns_device) and the split's own kernels
      = that ns_device minus the ns_device of (a)'s submit call, which runs the same pairing kernels over the same histories
IN ONE CALL (pageable memory):
  (c) numpy split_events + gather + tbc_pair_packed_batch, and its three pieces
  (d) tbc_pair_keyed_events, packed; (e) the same with out = NULL: the split alone
Each the median of `runs` after a warm-up; the verdicts of (a) and (b) and the outputs of (c) and (d) are compared.  One CHILD process
per size, each under its own `timeout -k 10`; the driver stops at the first non-zero status.
-> <out>/keyed_events_measure.txt (one JSON line per size, appended); the notes on them are in profiles/NOTES_pair_events.md.
  python scripts/gpu_keyed_events.py [--sizes 4096x1000,4096x10000] [--out profiles] [--runs 3] [--limit SECONDS]
THE TARGET SIZE (32,768 keys x 10k ops, 6.5 x 10^8 rows) and the parent commit's library: see big_child.
  python scripts/gpu_keyed_events.py --big 32768x10000 [--parent-lib PATH] [--runs 2] [--limit 900]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from jepsen_tigerbeetle_amd import _native as N, columns, synth  # noqa: E402

DISTINCT = 256


def say(*a):
    print(*a, flush=True)


def timed(fn, runs):
    fn()                                                    # warm-up
    ts, last = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        last = fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts), 4), last


def child(args):
    nk, m = (int(x) for x in args.size.split("x"))
    if N.lib().tbc_device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    base = [synth.register_events(n_ops=m, n_procs=64, seed=9000 + s, busy=0.1, n_values=4) for s in range(min(nk, DISTINCT))]
    evs = [base[h % len(base)] for h in range(nk)]
    lens = np.array([len(e) for e in evs], np.int64)
    hist = np.repeat(np.arange(nk), lens)
    pos = np.concatenate([np.arange(x) for x in lens])
    order = np.lexsort((hist, pos))                         # round-robin: a row of each key in turn
    _, cat = columns.concat_events(evs)
    word = columns.pack_events(cat)[order]                  # (a row's word does not depend on its neighbours)
    process = np.ascontiguousarray(cat.process[order])
    cat_type, cat_f, cat_a, cat_b = cat.type[order], cat.f[order], cat.a[order], cat.b[order]
    key = ((hist[order] * 2654435761) % (1 << 31)).astype(np.int32)      # (scattered key values)
    del cat, hist, pos, order
    n = len(key)
    r = {"keys": nk, "ops_per_key": m, "rows": n}
    say(f"# {nk} keys x {m} ops: {n} rows")
    pieces = {}

    def host_route():
        t0 = time.perf_counter()
        keys, ev_off, row_of = columns.split_events(key, key)
        t1 = time.perf_counter()
        w, p = word[row_of], process[row_of]
        t2 = time.perf_counter()
        st, out = columns.pair_events_batch_raw(ev_off, (w, p), columns=False, word=True)
        N.check_status(st)
        pieces.update(split_s=round(t1 - t0, 4), gather_s=round(t2 - t1, 4), pair_call_s=round(time.perf_counter() - t2, 4), pair_ns_device=out["ns_device"])
        out.update(keys=keys, ev_off=ev_off, row_of=row_of)
        return out

    def device_route():
        st, out = columns.pair_keyed_events_raw((word, process), key, columns=False, word=True)
        N.check_status(st)
        return out

    def split_alone():
        st, out = columns.pair_keyed_events_raw((word, process), key, pair=False)
        N.check_status(st)
        return out

    r["host_split_pair_s"], want = timed(host_route, args.runs)
    r.update({"host_" + k: v for k, v in pieces.items()})
    say(f"#   (c) numpy split + gather + tbc_pair_packed_batch {r['host_split_pair_s']} s: {pieces}")
    r["keyed_call_s"], got = timed(device_route, args.runs)
    r["keyed_ns_device"], r["keyed_bytes_in"] = got["ns_device"], got["bytes_in"]
    r["split_kernels_ms"] = round((got["ns_device"] - pieces["pair_ns_device"]) / 1e6, 3)
    say(f"#   (d) tbc_pair_keyed_events {r['keyed_call_s']} s: kernels {got['ns_device'] / 1e6:.2f} ms, of which the split {r['split_kernels_ms']} ms")
    for k in ("keys", "ev_off", "row_of", "op_off", "status", "n_process"):
        assert np.array_equal(got[k], want[k]), k
    T = want["n_ops"]
    assert got["n_ops"] == T and all(np.array_equal(got[k][:T], want[k][:T]) for k in ("word", "inv_pos", "ret_pos"))
    r["ops"] = int(T)
    r["split_only_call_s"], _ = timed(split_alone, args.runs)
    say(f"#   (e) the split alone {r['split_only_call_s']} s")
    del want
    # ---- into a batch
    from jepsen_tigerbeetle_amd import core
    ev = columns.EventColumns(np.ascontiguousarray(cat_type), process, np.ascontiguousarray(cat_f), np.ascontiguousarray(cat_a), np.ascontiguousarray(cat_b))
    st, raw = columns.pair_keyed_events_raw(ev, key)
    N.check_status(st)
    hists = columns.keyed_ops(raw)
    del raw
    opts = core.make_opts(time_limit_ms=600000, want_witness=False, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=4)
    with core.Batch(hists, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        b.run()
        verdicts = b.verdicts().copy()
        b.map_events(0), b.map_events(1), b.map_keyed_events(0)
        r["device_bytes"] = int(N.lib().tbc_batch_device_bytes(b._h))
        hp = {}

        def host_split_stream():
            t0 = time.perf_counter()
            keys, ev_off, row_of = columns.split_events(ev, key)
            t1 = time.perf_counter()
            moved, off = columns.take_events(ev, row_of), ev_off.astype(np.int64)
            evs = [columns.EventColumns(*[getattr(moved, c)[off[h]:off[h + 1]] for c in ("type", "process", "f", "a", "b")]) for h in range(len(keys))]
            t2 = time.perf_counter()
            b.stream_events(evs)
            b.run()
            hp.update(split_s=round(t1 - t0, 4), move_s=round(t2 - t1, 4), pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=b.events_report["ns_device"])

        kp = {}

        def keyed_stream():
            b.stream_keyed_events(ev, key)
            b.run()
            kp.update(pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=b.events_report["ns_device"], bytes_in=b.events_report["bytes_in"])

        r["batch_host_split_stream_run_s"], _ = timed(host_split_stream, args.runs)
        assert np.array_equal(b.verdicts(), verdicts)
        r.update({"batch_host_" + k: v for k, v in hp.items()})
        say(f"#   (a) numpy split + stream_events + run {r['batch_host_split_stream_run_s']} s: {hp}")
        r["batch_keyed_stream_run_s"], _ = timed(keyed_stream, args.runs)
        assert np.array_equal(b.verdicts(), verdicts)
        r.update({"batch_keyed_" + k: v for k, v in kp.items()})
        r["batch_split_kernels_ms"] = round((kp["ns_device"] - hp["ns_device"]) / 1e6, 3)

        def run_alone():
            b.run()

        r["run_alone_s"], _ = timed(run_alone, args.runs)
        say(f"#   (b) stream_keyed_events + run {r['batch_keyed_stream_run_s']} s: {kp}; the split's kernels {r['batch_split_kernels_ms']} ms; run alone {r['run_alone_s']} s")
    say(json.dumps(r))


def big_child(args):
    """THE TARGET SIZE, into a batch only: K keys x M ops as ONE history of K x L rows -- every key's history cut to the L rows of the
    shortest, so that the round-robin interleaving is a transpose and needs no sort to make.  With --lib (a library built from the
    parent commit) only what depends on the library is run: stream_events + run over the histories per key (what the numpy split
    gives); with this tree's library route (b), then route (a) whole, its numpy split and move timed ONCE without a warm-up.
    One JSON line per route."""
    import ctypes as C
    if args.lib:                                            # another build of the library: it lacks what this tree adds
        N.LIB_PATH = os.path.abspath(args.lib)
        probe = C.CDLL(N.LIB_PATH)
        for name in [x for x in N.SYMBOLS if not hasattr(probe, x)]:
            N.SYMBOLS.pop(name)
    from jepsen_tigerbeetle_amd import core
    nk, m = (int(x) for x in args.size.split("x"))
    if N.lib().tbc_device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    base = [synth.register_events(n_ops=m, n_procs=64, seed=9000 + s, busy=0.1, n_values=4) for s in range(min(nk, DISTINCT))]
    L = min(len(e) for e in base)
    base = [columns.take_events(e, np.arange(L)) for e in base]
    which = np.arange(nk) % len(base)
    hists = [columns.pair_events(e) for e in base]
    hists = [hists[w] for w in which]
    n = nk * L
    r0 = {"library": args.label, "keys": nk, "ops_per_key": m, "rows_per_key": L, "rows": n, "ops": int(sum(len(h) for h in hists))}
    say(f"# {args.label}: {nk} keys x {m} ops: {n} rows")
    opts = core.make_opts(time_limit_ms=600000, want_witness=False, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=4)
    with core.Batch(hists, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        b.run()
        verdicts = b.verdicts().copy()
        b.map_events(0, events_cap=n), b.map_events(1)
        per_key = [base[w] for w in which]                  # what split_events + the move give: key h's rows, in order

        def stream_run():
            b.stream_events(per_key)
            b.run()

        if args.lib:
            r = dict(r0, route="stream_events + run over the histories per key")
            r["stream_events_run_s"], _ = timed(stream_run, args.runs)
            r.update(pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=b.events_report["ns_device"])
            assert np.array_equal(b.verdicts(), verdicts)
            say(json.dumps(r))
            return
        # ---- this tree's library: the one history
        col = lambda name: np.ascontiguousarray(np.stack([getattr(e, name) for e in base])[which].T.reshape(-1))
        ev = columns.EventColumns(col("type"), col("process"), col("f"), col("a"), col("b"))
        key = np.tile(((np.arange(nk, dtype=np.int64) * 2654435761) % (1 << 31)).astype(np.int32), L)
        b.map_keyed_events(0)
        r = dict(r0, route="(b) stream_keyed_events + run", device_bytes=int(N.lib().tbc_batch_device_bytes(b._h)))

        def keyed_stream():
            b.stream_keyed_events(ev, key)
            b.run()

        r["stream_keyed_events_run_s"], _ = timed(keyed_stream, args.runs)
        rep = b.events_report
        r.update(pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=rep["ns_device"], bytes_in=rep["bytes_in"], n_keys=rep["n_keys"])
        assert np.array_equal(b.verdicts(), verdicts) and rep["n_keys"] == nk
        r["run_alone_s"], _ = timed(b.run, args.runs)
        say(json.dumps(r))
        # ---- route (a), once
        r = dict(r0, route="(a) numpy split_events + move + stream_events + run, once, no warm-up")
        t0 = time.perf_counter()
        keys, ev_off, row_of = columns.split_events(ev, key)
        t1 = time.perf_counter()
        moved, off = columns.take_events(ev, row_of), ev_off.astype(np.int64)
        evs = [columns.EventColumns(*[getattr(moved, c)[off[h]:off[h + 1]] for c in ("type", "process", "f", "a", "b")]) for h in range(len(keys))]
        t2 = time.perf_counter()
        b.stream_events(evs)
        b.run()
        t3 = time.perf_counter()
        assert np.array_equal(b.verdicts(), verdicts)
        r.update(split_s=round(t1 - t0, 3), move_s=round(t2 - t1, 3), stream_events_run_s=round(t3 - t2, 4), total_s=round(t3 - t0, 3),
                 pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=b.events_report["ns_device"])
        r["split_kernels_ms"] = round((rep["ns_device"] - r["ns_device"]) / 1e6, 3)
        say(json.dumps(r))
        del evs, moved
        r = dict(r0, route="stream_events + run over the histories per key")
        r["stream_events_run_s"], _ = timed(stream_run, args.runs)
        r.update(pack_s=round(b.pack_s, 4), submit_s=round(b.submit_s, 4), ns_device=b.events_report["ns_device"])
        say(json.dumps(r))


def big_main(args):
    """--big KEYSxOPS [--parent-lib PATH]: the parent's library first (what of route (a) depends on it), then this tree's"""
    os.makedirs(args.out, exist_ok=True)
    for label, lib in ([("parent", args.parent_lib)] if args.parent_lib else []) + [("tree", None)]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--big-child", "--size", args.big, "--runs", str(args.runs), "--label", label]
        if lib:
            cmd += ["--lib", lib]
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as p:
            for line in p.stdout:
                say(line.rstrip("\n"))
                if line.startswith("{"):
                    with open(os.path.join(args.out, "keyed_events_measure.txt"), "a") as f:
                        f.write(line.strip() + "\n")
        if p.returncode != 0:                               # (a fault, a hang, a failed assertion: nothing more is started)
            raise SystemExit(f"the child for {label}, {args.big} ended with status {p.returncode}: stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x1000,4096x10000")
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--size", default="", help="(a child) the one size to measure, KEYSxOPS")
    ap.add_argument("--big", default="", help="KEYSxOPS: the target size, the batch routes only (big_child)")
    ap.add_argument("--parent-lib", default=None, help="libtbcheck.so built from the parent commit (with --big)")
    ap.add_argument("--big-child", action="store_true", help="(a child of --big)")
    ap.add_argument("--lib", default=None, help="(a child) the library to load instead of the tree's")
    ap.add_argument("--label", default="tree", help="(a child) what the lines call their library")
    args = ap.parse_args()
    if args.big_child:
        return big_child(args)
    if args.big:
        return big_main(args)
    if args.size:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    for size in args.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--size", size, "--runs", str(args.runs)]
        last = ""
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as p:
            for line in p.stdout:
                say(line.rstrip("\n"))
                last = line if line.strip() else last
        if p.returncode != 0:                               # (a fault, a hang, a failed assertion: nothing more is started)
            raise SystemExit(f"the child for {size} ended with status {p.returncode}: stopping")
        with open(os.path.join(args.out, "keyed_events_measure.txt"), "a") as f:
            f.write(last.strip() + "\n")


if __name__ == "__main__":
    main()

"""The cycle search over a ledger's reads (jepsen/ledger.py CycleSearch), cycles_numpy's reduction against the device route, on a synthetic
ledger from the test generator (tests/ledger_histories.py random_ledger): 64 workers, 50k transfers, 50k reads of 8 accounts, the shape
of profiles/ledger_snapshots_measure_50k.txt.  One process; every raw line is printed as it is measured and written to --out
(profiles/ledger_cycles_measure_50k.txt).

    python scripts/gpu_ledger_cycles.py [--transfers 50000] [--reads 50000] [--workers 64] [--reps 7] [--out FILE]

Three cases:
  a  the valid history, every read complete: no core, no matrix, no closure.  tbc_ledger_snapshots alone is timed on the same columns
     too, since the new call repeats its layout and sort
  b  the same history with one account dropped from 1 % of the reads (seeded): still valid, the partial reads are the core
  c  b with three partial reads appended that form a 3-cycle among themselves
Both routes start from ready LedgerColumns and end with the arrays; they are run alternately, `reps` times each after one warm-up each,
and the medians are reported beside the raw times.  The arrays and summaries of both routes are compared before any time is reported."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ledger_histories as G  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import ledger as L  # noqa: E402


def is_ok_read(op):
    return isinstance(op.get("process"), int) and op["type"] == "ok" and L.op_txn_f(op) == "r"


def measure(say, case, h, o, reps, snapshots_too):
    accounts = o["accounts"]
    t = time.perf_counter()
    cols = L.LedgerColumns(h)
    say({"case": case, "ops": len(h), "reads": int(len(cols.read_ops)), "micro_ops": int(len(cols.mop_id)), "s_ledger_columns": round(time.perf_counter() - t, 3)})
    t_np, t_dev, t_snap, ns, ns_snap, host, dev = [], [], [], [], [], None, None
    for rep in range(reps + 1):                                              # (rep 0 warms both up: the library loaded, the device initialised)
        t = time.perf_counter(); host = L.cycles_dense_numpy(*L._snap_dense(cols, accounts), *L._cyc_times(cols)); t_host = time.perf_counter() - t
        t = time.perf_counter(); dev = L.check_cycles_native(cols, accounts); t1 = time.perf_counter() - t
        if snapshots_too:
            t = time.perf_counter(); snap = L.check_snapshots_native(cols, accounts); t2 = time.perf_counter() - t
        if rep:
            t_np.append(t_host); t_dev.append(t1); ns.append(dev["summary"]["ns_device"])
            if snapshots_too:
                t_snap.append(t2); ns_snap.append(snap["summary"]["ns_device"])
    for k in L.CYC_ARRAYS:
        assert np.array_equal(host[k], dev[k]), k
    s = dev["summary"]
    assert {k: v for k, v in s.items() if k not in ("ns_device", "bytes_in")} == host["summary"]
    line = {"case": case, "s_cycles_numpy": [round(x, 5) for x in t_np], "s_tbc_ledger_cycles": [round(x, 5) for x in t_dev],
            "median_s_cycles_numpy": round(statistics.median(t_np), 5), "median_s_tbc_ledger_cycles": round(statistics.median(t_dev), 5),
            "ns_device": ns, "median_ns_device": int(statistics.median(ns)), "bytes_in": s["bytes_in"], "checked": s["n_checked"], "valid": s["valid"],
            "n_partial": s["n_partial"], "n_core": s["n_core"], "n_on_cycle": s["n_on_cycle"], "n_components": s["n_components"],
            "largest_size": s["largest_size"], "closure_rounds": s["closure_rounds"]}
    if snapshots_too:
        line.update({"s_tbc_ledger_snapshots": [round(x, 5) for x in t_snap], "median_s_tbc_ledger_snapshots": round(statistics.median(t_snap), 5),
                     "ns_device_snapshots": ns_snap, "median_ns_device_snapshots": int(statistics.median(ns_snap))})
    say(line)
    t = time.perf_counter()
    m = L.cycles_result_map(h, cols, dev, accounts)
    say({"case": case, "s_result_map": round(time.perf_counter() - t, 4), "valid?": m["valid?"], "witness_steps": None if m["witness"] is None else len(m["witness"])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", type=int, default=50000)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--workers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_cycles_measure_50k.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def say(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    t = time.perf_counter()
    h, o = G.random_ledger(1, workers=a.workers, transfers=a.transfers, reads=a.reads)
    say({"shape": {"workers": a.workers, "transfers": a.transfers, "reads": a.reads, "ops": len(h)}, "s_generate": round(time.perf_counter() - t, 3)})
    if "a" in a.cases:
        measure(say, "a every read complete", h, o, a.reps, True)
    rng = random.Random(2)

    def drop(op):
        k = rng.randrange(len(op["value"]))
        return dict(op, value=op["value"][:k] + op["value"][k + 1:]) if len(op["value"]) > 1 else op

    hb = [drop(op) if is_ok_read(op) and rng.random() < 0.01 else op for op in h]
    if "b" in a.cases:
        measure(say, "b 1 % partial reads, valid", hb, o, a.reps, False)
    if "c" in a.cases:
        last = next(op for op in reversed(h) if is_ok_read(op))
        top = {i: m for _f, i, m in last["value"]}
        a1, a2, a3 = o["accounts"][:3]
        bump = lambda acct, n: ["r", acct, {"credits-posted": top[acct]["credits-posted"] + n, "debits-posted": top[acct]["debits-posted"] + n}]
        rows = [[bump(a1, 5), bump(a2, 1)], [bump(a2, 2), bump(a3, 1)], [bump(a3, 2), bump(a1, 4)]]
        hc, base = list(hb), 1 + max(op["process"] for op in h if isinstance(op.get("process"), int))
        for k, row in enumerate(rows):
            hc.append({"type": "invoke", "f": "txn", "value": [["r", m[1], None] for m in row], "process": base + k, "index": len(hc), "time": hc[-1]["time"] + 1})
        for k, row in enumerate(rows):
            hc.append({"type": "ok", "f": "txn", "value": row, "process": base + k, "index": len(hc), "time": hc[-1]["time"] + 1})
        measure(say, "c 1 % partial reads and a planted 3-cycle", hc, o, a.reps, False)


if __name__ == "__main__":
    main()

"""The snapshot order of a ledger's reads (jepsen/ledger.py SnapshotOrder), snapshots_numpy against the device route, on a synthetic
ledger from the test generator (tests/ledger_histories.py random_ledger): 64 workers, 50k transfers, 50k reads of 8 accounts, the shape
of profiles/ledger_realtime_measure_50k.txt.  One process; every raw line is printed as it is measured and written to --out
(profiles/ledger_snapshots_measure_50k.txt).

    python scripts/gpu_ledger_snapshots.py [--transfers 50000] [--reads 50000] [--workers 64] [--reps 7] [--out FILE]

Four cases:
  a  the valid history: no candidate, no pair kernel
  b  the same history with 32 forks planted (tests/ledger_snapshot_histories.py plant_forks): 64 candidates
  c  the same history with one account's micro-op nil in every read: every read is partial, so every read is a candidate -- the cost
     of the quadratic pass at this size, without any switch.  snapshots_numpy compares every candidate with every read in a Python
     loop, minutes at this size: it is timed ONCE here, the device `reps` times.
  d  the valid history at half the reads
Both routes start from ready LedgerColumns and end with the arrays; they are run alternately, `reps` times each after one warm-up each,
and the medians are reported beside the raw times.  The arrays and summaries of both routes are compared before any time is reported.
The last line is ns_device(a) / ns_device(d): about 2 for an n log n route, 4 for a quadratic one."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ledger_histories as G  # noqa: E402
import ledger_snapshot_histories as S  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import ledger as L  # noqa: E402


def measure(say, case, h, o, reps, numpy_reps):
    accounts = o["accounts"]
    t = time.perf_counter()
    cols = L.LedgerColumns(h)
    say({"case": case, "ops": len(h), "reads": int(len(cols.read_ops)), "micro_ops": int(len(cols.mop_id)), "s_ledger_columns": round(time.perf_counter() - t, 3)})
    t_np, t_dev, ns, host, dev = [], [], [], None, None
    for rep in range(reps + 1):                                              # (rep 0 warms both up: the library loaded, the device initialised)
        if rep <= numpy_reps:
            t = time.perf_counter(); host = L.snapshots_dense_numpy(*L._snap_dense(cols, accounts)); t_host = time.perf_counter() - t
        t = time.perf_counter(); dev = L.check_snapshots_native(cols, accounts); t1 = time.perf_counter() - t
        if rep or numpy_reps == 0:
            if rep <= numpy_reps:
                t_np.append(t_host)
            t_dev.append(t1); ns.append(dev["summary"]["ns_device"])
    for k in ("count", "first", "key", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    s = dev["summary"]
    assert {k: v for k, v in s.items() if k not in ("ns_device", "bytes_in")} == host["summary"]
    rd = (cols.type == L.N.LEDGER_T_OK) & (cols.kind == L.N.LEDGER_K_READ)
    say({"case": case, "s_snapshots_numpy": [round(x, 5) for x in t_np], "s_tbc_ledger_snapshots": [round(x, 5) for x in t_dev],
         "median_s_snapshots_numpy": round(statistics.median(t_np), 5), "median_s_tbc_ledger_snapshots": round(statistics.median(t_dev), 5),
         "ns_device": ns, "median_ns_device": int(statistics.median(ns)), "bytes_in": s["bytes_in"],
         "read_micro_ops": int((cols.mop_off[1:][rd] - cols.mop_off[:-1][rd]).sum()), "checked": s["n_checked"], "valid": s["valid"],
         "n_partial": s["n_partial"], "n_candidates": s["n_candidates"], "skewed": s["skewed"]["count"], "n_pairs": s["n_pairs"]})
    t = time.perf_counter()
    m = L.snapshots_result_map(h, cols, dev, accounts)
    say({"case": case, "s_result_map": round(time.perf_counter() - t, 4), "valid?": m["valid?"], "exact?": m["exact?"]})
    return int(statistics.median(ns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", type=int, default=50000)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--workers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--forks", type=int, default=32)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_snapshots_measure_50k.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def say(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    def ledger(reads):
        t = time.perf_counter()
        h, o = G.random_ledger(1, workers=a.workers, transfers=a.transfers, reads=reads)
        funded = o["total-amount"] // len(o["accounts"])                     # (the generator funds every account with credits)
        o = dict(o, initial={acct: {"credits-posted": funded, "debits-posted": 0} for acct in o["accounts"]})
        say({"shape": {"workers": a.workers, "transfers": a.transfers, "reads": reads, "ops": len(h)}, "s_generate": round(time.perf_counter() - t, 3)})
        return h, o

    h, o = ledger(a.reads)
    ns = {}
    if "a" in a.cases:
        ns["a"] = measure(say, "a valid", h, o, a.reps, a.reps)
    if "b" in a.cases:
        ns["b"] = measure(say, f"b {a.forks} forks", S.plant_forks(h, o, a.forks)[0], o, a.reps, a.reps)
    if "c" in a.cases:
        first = o["accounts"][0]
        nil = lambda op: dict(op, value=[[f, i, None if i == first else m] for f, i, m in op["value"]])
        hc = [nil(op) if isinstance(op.get("process"), int) and op["type"] == "ok" and L.op_txn_f(op) == "r" else op for op in h]
        ns["c"] = measure(say, "c every read partial", hc, o, min(a.reps, 3), 0)
    if "d" in a.cases:
        h, o = ledger(a.reads // 2)
        ns["d"] = measure(say, "d valid, half the reads", h, o, a.reps, a.reps)
    if "a" in ns and "d" in ns:
        say({"ns_device_a_over_d": round(ns["a"] / ns["d"], 3)})


if __name__ == "__main__":
    main()

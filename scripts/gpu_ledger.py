"""The ledger workload's checkers, host statement against device route, on synthetic ledgers from the test generator
(tests/ledger_histories.py random_ledger): 64 workers, N transfers, 50k reads of 8 accounts, the full final phase -- every worker's final
lookup returns every transfer, so the lookups hold 64 x N micro-ops.  One process; every raw line is printed as it is measured.

    python scripts/gpu_ledger.py [--transfers 50000 500000] [--reads 50000] [--workers 64] [--reps 3]

Per shape: the host statement (SI, lookup-transfers, final-reads of jepsen/ledger.py, one after the other), LedgerColumns +
check_columns as a whole call, the bare tbc_ledger_check over ready columns, and its ns_device and bytes_in.  The results of both
routes are compared before any time is reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ledger_histories as G  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import ledger as L  # noqa: E402


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", type=int, nargs="+", default=[50000, 500000])
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--workers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L.check_columns(G.random_ledger(0, transfers=5, reads=5)[0])          # (the library loaded, the device initialised)
    for n in a.transfers:
        t = time.perf_counter()
        h, o = G.random_ledger(1, workers=a.workers, transfers=n, reads=a.reads)
        print(json.dumps({"shape": {"workers": a.workers, "transfers": n, "reads": a.reads, "ops": len(h)}, "s_generate": round(time.perf_counter() - t, 3)}), flush=True)
        host, t_host = timed(lambda: {"SI": L.BankChecker(o).check(o, h), "lookup-transfers": L.LookupAllInvokedTransfers().check(o, h),
                                      "final-reads": L.FinalReads().check(o, h)}, 1 if n > 100000 else a.reps)
        print(json.dumps({"transfers": n, "s_host_statement": [round(x, 4) for x in t_host]}), flush=True)
        dev, t_whole = timed(lambda: L.check_columns(h, o), a.reps)
        assert dev == host, "the device route and the host statement disagree"
        print(json.dumps({"transfers": n, "s_columns_and_check_columns": [round(x, 4) for x in t_whole]}), flush=True)
        cols, t_cols = timed(lambda: L.LedgerColumns(h, o["total-amount"]), 1)
        raw, t_bare = timed(lambda: L.check_native(cols, o["accounts"], False), a.reps + 2)
        s = raw["summary"]
        print(json.dumps({"transfers": n, "micro_ops": int(len(cols.mop_id)), "lookup_micro_ops": int(s["n_final_lookups"]) * int(s["n_transfers"]),
                          "s_ledger_columns": [round(x, 4) for x in t_cols], "s_tbc_ledger_check": [round(x, 5) for x in t_bare],
                          "ns_device": s["ns_device"], "bytes_in": s["bytes_in"], "valid": [s["valid_si"], s["valid_lookups"], s["valid_final_reads"]]}), flush=True)
        del h, cols, dev, host, raw


if __name__ == "__main__":
    main()

"""The ledger's realtime bounds (jepsen/ledger.py RealtimeBounds), realtime_numpy against the device route, on a synthetic ledger from
the test generator (tests/ledger_histories.py random_ledger): 64 workers, N transfers, 50k reads of 8 accounts, the shape of
profiles/NOTES_ledger.md.  One process; every raw line is printed as it is measured.

    python scripts/gpu_ledger_realtime.py [--transfers 50000] [--reads 50000] [--workers 64] [--reps 7]

Both routes start from ready LedgerColumns (the flattening is the same Python pass for either) and end with the arrays; they are run
ALTERNATELY, `reps` times each after one warm-up each, and the medians are reported beside the raw times.  The arrays of both routes are
compared before any time is reported.  Also printed: ns_device, bytes_in, and the bytes the query kernel must move at least (from the
layout: per read micro-op its id, both counters and flag in, six bounds out; per list entry its position and running value in once),
to set against the query kernel's time in a kernel trace of this script."""
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
from jepsen_tigerbeetle_amd.jepsen import ledger as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", type=int, nargs="+", default=[50000])
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--workers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    for n in a.transfers:
        t = time.perf_counter()
        h, o = G.random_ledger(1, workers=a.workers, transfers=n, reads=a.reads)
        funded = o["total-amount"] // len(o["accounts"])                     # (the generator funds every account with credits)
        o = dict(o, initial={acct: {"credits-posted": funded, "debits-posted": 0} for acct in o["accounts"]})
        accounts, init, apply_ok = L._rt_opts(None, o)
        print(json.dumps({"shape": {"workers": a.workers, "transfers": n, "reads": a.reads, "ops": len(h)}, "s_generate": round(time.perf_counter() - t, 3)}), flush=True)
        t = time.perf_counter()
        cols = L.LedgerColumns(h)
        print(json.dumps({"transfers": n, "micro_ops": int(len(cols.mop_id)), "s_ledger_columns": round(time.perf_counter() - t, 3)}), flush=True)
        t_np, t_dev, host, dev = [], [], None, None
        for rep in range(a.reps + 1):                                        # (rep 0 warms both up: the library loaded, the device initialised)
            t = time.perf_counter(); host = L.realtime_numpy_columns(cols, accounts, init, apply_ok); t1 = time.perf_counter()
            dev = L.check_realtime_native(cols, accounts, init, apply_ok); t2 = time.perf_counter()
            if rep:
                t_np.append(t1 - t); t_dev.append(t2 - t1)
        for k in ("bits", "miss", "lo", "hi", "floor"):
            assert np.array_equal(host[k], dev[k]), k
        s = dev["summary"]
        assert {k: v for k, v in s.items() if k not in ("ns_device", "bytes_in")} == host["summary"]
        read_mops = len(dev["lo"])
        tr = (cols.type == L.N.LEDGER_T_INVOKE) & (cols.kind == L.N.LEDGER_K_TRANSFER)
        transfer_mops = int((cols.mop_off[1:][tr] - cols.mop_off[:-1][tr]).sum())
        entries = 2 * s["n_checked"] + 2 * 2 * transfer_mops                 # (the reads' lists, and at most both transfers' lists)
        print(json.dumps({"transfers": n, "s_realtime_numpy": [round(x, 5) for x in t_np], "s_tbc_ledger_realtime": [round(x, 5) for x in t_dev],
                          "median_s_realtime_numpy": round(statistics.median(t_np), 5), "median_s_tbc_ledger_realtime": round(statistics.median(t_dev), 5),
                          "ns_device": s["ns_device"], "bytes_in": s["bytes_in"], "read_micro_ops": read_mops, "checked": s["n_checked"],
                          "valid": s["valid"], "error_count": s["error_count"], "n_definite": s["n_definite"], "n_possible": s["n_possible"],
                          "query_bytes_at_least": 25 * read_mops + 48 * read_mops + 12 * entries}), flush=True)
        t = time.perf_counter()
        m = L.realtime_result_map(h, cols, dev, accounts, init, apply_ok)
        print(json.dumps({"transfers": n, "s_result_map": round(time.perf_counter() - t, 4), "valid?": m["valid?"]}), flush=True)


if __name__ == "__main__":
    main()

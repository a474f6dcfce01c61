"""The journal audit of a ledger's lookups (jepsen/ledger.py JournalAudit), journal_numpy against the device route, on a synthetic ledger
from the test generator (tests/ledger_journal_histories.py journal_ledger): 64 workers, 50k transfers (1 to 3 micro-ops each), 50k reads
of 8 accounts, 16 mid-history lookups and 64 final ones -- each final lookup returns the whole journal.  One process; every raw line is
printed as it is measured and written to --out (profiles/ledger_journal_measure_50k.txt).

    python scripts/gpu_ledger_journal.py [--transfers 50000] [--reads 50000] [--workers 64] [--mid 16] [--reps 5] [--out FILE]

Four cases:
  a  the valid history
  b  the same history with the plants (altered, early, lost, vanished, ahead-of-journal; tests/ledger_journal_histories.py plant)
  c  half the transfers
  d  the history of (a) with half the final lookups (32 workers make final ops)
Both routes start from ready LedgerColumns and end with the arrays; they are run alternately, `reps` times each after one warm-up each,
and the medians are reported beside the raw times.  The arrays and summaries of both routes are compared before any time is reported.
Per case: journal_numpy's time, bytes_in, and 33 B x entries / ns_device as a fraction of the 6.29 TB/s a float4 copy reaches on the
MI355X (the whole call's kernels in the denominator, not the entries kernel alone: an upper bound on its distance from streaming).
The last line is ns_device(a) / ns_device(c) and ns_device(a) / ns_device(d): each about 2 if the call is linear in entries."""
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

import ledger_journal_histories as J  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import ledger as L  # noqa: E402

HBM_COPY_BYTES_PER_NS = 6290.0                      # 6.29 TB/s, measured float4 copy


def measure(say, case, h, o, reps):
    accounts, init, apply_ok = L._rt_opts(None, o)
    t = time.perf_counter()
    cols = L.LedgerColumns(h)
    E, NL, R, M = L.journal_shapes(cols)
    say({"case": case, "ops": len(h), "entries": E, "lookups": NL, "reads": R, "transfer_micro_ops": M, "s_ledger_columns": round(time.perf_counter() - t, 3)})
    t_np, t_dev, ns, host, dev = [], [], [], None, None
    for rep in range(reps + 1):                                              # (rep 0 warms both up: the library loaded, the device initialised)
        t = time.perf_counter(); host = L.journal_numpy_columns(cols, accounts, init, apply_ok); t_host = time.perf_counter() - t
        t = time.perf_counter(); dev = L.check_journal_native(cols, accounts, init, apply_ok); t1 = time.perf_counter() - t
        if rep:
            t_np.append(t_host); t_dev.append(t1); ns.append(dev["summary"]["ns_device"])
    for k in L.JN_ARRAYS:
        assert np.array_equal(host[k], dev[k]), k
    s = dev["summary"]
    assert {k: v for k, v in s.items() if k not in ("ns_device", "bytes_in")} == host["summary"]
    med = int(statistics.median(ns))
    say({"case": case, "s_journal_numpy": [round(x, 4) for x in t_np], "s_tbc_ledger_journal": [round(x, 4) for x in t_dev],
         "median_s_journal_numpy": round(statistics.median(t_np), 4), "median_s_tbc_ledger_journal": round(statistics.median(t_dev), 4),
         "ns_device": ns, "median_ns_device": med, "bytes_in": s["bytes_in"], "entry_bytes_per_ns": round(33 * E / med, 2),
         "fraction_of_hbm_copy": round(33 * E / med / HBM_COPY_BYTES_PER_NS, 4), "checked": s["n_checked"], "records": s["n_records"],
         "valid": s["valid"], "totals": {k: v for k, v in s["totals"].items() if v}})
    t = time.perf_counter()
    m = L.journal_result_map(h, cols, dev)
    say({"case": case, "s_result_map": round(time.perf_counter() - t, 4), "valid?": m["valid?"], "errors": sorted(m["errors"])})
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", type=int, default=50000)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--workers", type=int, default=64)
    ap.add_argument("--mid", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_journal_measure_50k.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def say(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    def ledger(transfers, finals):
        t = time.perf_counter()
        kinds = ["t"] * transfers + ["r"] * a.reads
        np.random.RandomState(1).shuffle(kinds)
        step = len(kinds) // (a.mid + 1)
        for k in range(a.mid, 0, -1):                                        # the mid-history lookups, evenly spaced
            kinds.insert(k * step, "l")
        h, o, meta = J.journal_ledger(1, workers=a.workers, kinds=kinds, finals=finals)
        say({"shape": {"workers": a.workers, "transfers": transfers, "reads": a.reads, "mid_lookups": a.mid, "final_lookups": finals, "ops": len(h)},
             "s_generate": round(time.perf_counter() - t, 3)})
        return h, o, meta

    ns = {}
    h, o, meta = ledger(a.transfers, a.workers)
    if "a" in a.cases:
        ns["a"] = measure(say, "a valid", h, o, a.reps)
    if "b" in a.cases:
        hb = h
        for name in ("altered", "early", "lost", "vanished", "ahead-of-journal"):
            hb, _ = J.plant(hb, meta, name)
        ns["b"] = measure(say, "b planted", hb, o, a.reps)
    if "d" in a.cases:
        ns["d"] = measure(say, "d half the final lookups", *ledger(a.transfers, a.workers // 2)[:2], a.reps)
    del h, meta
    if "c" in a.cases:
        ns["c"] = measure(say, "c half the transfers", *ledger(a.transfers // 2, a.workers)[:2], a.reps)
    if "a" in ns and "c" in ns and "d" in ns:
        say({"ns_device_a_over_c": round(ns["a"] / ns["c"], 3), "ns_device_a_over_d": round(ns["a"] / ns["d"], 3)})


if __name__ == "__main__":
    main()

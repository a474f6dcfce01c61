"""set-full's verdict: what it costs after the scan, on the host (result_map over the three indices) and on the device
(tbc_setfull_keys_results + result_from_device).

The script runs on a build WITH the device results and on one WITHOUT (the parent: only what it has is measured), one process per build;
compare the two outputs.  Shapes:
  bench  the bench's set-full key: 262,144 elements x 32,768 reads (scripts/gpu_setfull_keys.streaming_key)
  a      config 3 of BASELINE.json: 5 keys, ~50k ops in all        }  as scripts/gpu_setfull_keys.py
  b      256 keys x 2k ops                                          }
Per shape, medians of --reps runs after warm-up, every raw line kept ("raw": the per-rep values):
  scan_ns            ns_scan of tbc_setfull_keys_run
  host_map_ms        result_map over every key after the scan (the host statement; what the parent's check pays)
  verdict_ms         encodings -> result maps: keyed create + (run + result_map | results + result_from_device) + destroy
  check_keys_ms      the whole check_keys call, encoding included (a, b)
  results_scan_ns / results_ns / device_map_ms       (builds with the device results) ns_scan and ns_results of one
                     tbc_setfull_keys_results call, and result_from_device over every key

  python scripts/gpu_setfull_results.py [--shapes bench,a,b] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from helpers import set_history  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import set_full as sf  # noqa: E402
from gpu_setfull_keys import streaming_key  # noqa: E402

DEVICE = hasattr(sf, "result_from_device")


def as_encoded(a):
    """What result_map / result_from_device read of an `Encoded`, for a key built as arrays: elements named by their numbers, no :time."""
    n = int(max(a.add_ok.max(), a.read_ok.max())) + 1
    a.elements, a.times, a.has_time, a.duplicated = list(range(a.E)), dict(zip(range(n), range(n))), False, {}
    a.op_time, a.unit, a.n_ops = None, 1, n
    return a


def shape(name):
    if name == "bench":
        return None, [as_encoded(streaming_key(262_144, 32_768, 1))]
    hists = [set_history(10_000, 10, 300 + k, busy=0.3, info=0.02) for k in range(5)] if name == "a" else \
            [set_history(2_000, 6, 500 + k, busy=0.3, info=0.02) for k in range(256)]
    return dict(enumerate(hists)), [sf.Encoded(h) for h in hists]


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t), out


def verdict_host(encs):
    with sf.KeyedScan(encs) as ks:
        per, _ = ks.run()
    return [sf.result_map(e, st, True) for e, st in zip(encs, per)]


def verdict_device(encs):
    times = None if all(e.op_time is None for e in encs) else [sf._time_column(e) for e in encs]
    with sf.KeyedScan(encs) as ks:
        per, _ = ks.results(times, encs[0].unit, True)
    return [sf.result_from_device(e, d) for e, d in zip(encs, per)]


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench,a,b")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    for name in args.shapes.split(","):
        hists, encs = shape(name)
        raw = {k: [] for k in ("scan_ns", "host_map_ms", "verdict_ms", "check_keys_ms", "results_scan_ns", "results_ns", "device_map_ms")}
        if DEVICE:                                   # correctness first: the device's maps are the host statement's
            assert verdict_device(encs) == verdict_host(encs), name
        with sf.KeyedScan(encs) as ks:
            times = None
            if DEVICE:
                times = None if all(e.op_time is None for e in encs) else [sf._time_column(e) for e in encs]
            for rep in range(args.warmup + args.reps):
                per, tot = ks.run()
                ms, _ = timed(lambda: [sf.result_map(e, st, True) for e, st in zip(encs, per)])
                row = {"scan_ns": tot["ns_scan"], "host_map_ms": ms}
                if DEVICE:
                    dev, dtot = ks.results(times, encs[0].unit, True)
                    row["results_scan_ns"], row["results_ns"] = dtot["ns_scan"], dtot["ns_results"]
                    row["device_map_ms"] = timed(lambda: [sf.result_from_device(e, d) for e, d in zip(encs, dev)])[0]
                if rep >= args.warmup:
                    for k, v in row.items():
                        raw[k].append(v)
        for rep in range(args.warmup + args.reps):
            ms = timed(lambda: (verdict_device if DEVICE else verdict_host)(encs))[0]
            ck = timed(lambda: sf.check_keys(hists, True))[0] if hists is not None else None
            if rep >= args.warmup:
                raw["verdict_ms"].append(ms)
                if ck is not None:
                    raw["check_keys_ms"].append(ck)
        rec = {"shape": name, "device_results": DEVICE, "keys": len(encs), "elements": int(sum(e.E for e in encs)), "reads": int(sum(e.R for e in encs))}
        for k, v in raw.items():
            if v:
                rec[k] = {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        rec["raw"] = {k: [round(x, 4) for x in v] for k, v in raw.items() if v}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

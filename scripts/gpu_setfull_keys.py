"""set-full over many keys: one keyed object (tbc_setfull_keys_*) against the loop of single-key Scans on the same keys.

Shapes (ISSUE: batch set-full across independent keys):
  a  config 3 of BASELINE.json: 5 keys, ~50k ops in all (tests/helpers.set_history)
  b  256 keys x 2k ops (tests/helpers.set_history)
  c  16 keys x 16,384 elements x 16,384 reads, the streaming shape (numpy, compact reads as bench.py's set-full leg builds them)
Per shape: host encode time; keyed create + run + destroy and the per-key loop end to end (medians after warm-up, min / max as the
spread); for c the keyed scan's bytes over its event time as a share of 8 TB/s.  Before any timing the keyed indices are checked
equal to the per-key ones.  One JSON line per shape.

  python scripts/gpu_setfull_keys.py [--shapes abc] [--reps 15]
  python scripts/gpu_setfull_keys.py --trace a     one keyed create + run (for rocprofv3 --kernel-trace --stats: launches per run)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import set_history  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import set_full as sf  # noqa: E402

HBM = 8e12


class Arr:
    pass


def streaming_key(E, R, seed):
    """E elements, R reads: read r holds every element invoked before it completed, but a hole in 1 % of the reads (compact form)."""
    rng = np.random.default_rng(seed)
    a = Arr()
    a.E, a.R, a.wpr = E, R, (E + 31) // 32
    a.add_invoke = (np.arange(E, dtype=np.int64) * 4).astype(np.uint32)
    a.add_ok = (a.add_invoke + 1).astype(np.uint32)
    a.read_invoke = (np.arange(R, dtype=np.int64) * 4 * E // R + 2).astype(np.uint32)
    a.read_ok = (a.read_invoke.astype(np.int64) + 4 * rng.integers(0, 64, R) + 1).astype(np.uint32)
    a.top = np.minimum(E, np.searchsorted(a.add_invoke, a.read_ok)).astype(np.uint32)
    n_h = ((rng.random(R) < 0.01) & (a.top > 0)).astype(np.int64)
    a.exc_off = np.concatenate([[0], np.cumsum(n_h)]).astype(np.uint64)
    rows = np.nonzero(n_h)[0]
    a.exc = (rng.integers(0, a.top[rows].astype(np.int64)) if len(rows) else np.zeros(0, np.int64)).astype(np.uint32)
    return a


def shape(name):
    if name == "a":
        hists = [set_history(10_000, 10, 300 + k, busy=0.3, info=0.02) for k in range(5)]
    elif name == "b":
        hists = [set_history(2_000, 6, 500 + k, busy=0.3, info=0.02) for k in range(256)]
    else:
        return [streaming_key(16_384, 16_384, 700 + k) for k in range(16)], None
    t = time.perf_counter()
    encs = [sf.Encoded(h) for h in hists]
    return encs, time.perf_counter() - t


def keyed_once(encs):
    t = time.perf_counter()
    with sf.KeyedScan(encs) as ks:
        per, tot = ks.run()
    return time.perf_counter() - t, per, tot


def loop_once(encs):
    t = time.perf_counter()
    out = []
    for e in encs:
        with sf.Scan(e, rows=True) as s:
            out.append(s.run())
    return time.perf_counter() - t, out


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(1e3 * xs[len(xs) // 2], 4), "min_ms": round(1e3 * xs[0], 4), "max_ms": round(1e3 * xs[-1], 4), "n": len(xs)}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default=None, help="one keyed create + run of this shape (a / b), nothing else")
    args = ap.parse_args()
    if args.trace:
        encs, _ = shape(args.trace)
        _, per, _ = keyed_once(encs)
        print(json.dumps({"trace": args.trace, "keys": len(encs), "elements": int(sum(len(p["known"]) for p in per))}))
        return
    for name in args.shapes:
        encs, enc_s = shape(name)
        # correctness first: keyed == per key, bit for bit
        _, per, tot = keyed_once(encs)
        _, single = loop_once(encs)
        for i, (p, s) in enumerate(zip(per, single)):
            for f in ("known", "last_present", "last_absent"):
                assert np.array_equal(p[f], s[f]), (name, i, f)
        for _ in range(args.warmup):
            keyed_once(encs)
            loop_once(encs)
        kt, lt, one, scan_ns = [], [], [], []
        for _ in range(args.reps):                   # alternated, so that drift hits both alike
            dt, _, tt = keyed_once(encs)
            kt.append(dt)
            scan_ns.append(tt["ns_scan"])
            lt.append(loop_once(encs)[0])
            one.append(loop_once(encs[:1])[0])
        rec = {"shape": name, "keys": len(encs), "elements": int(sum(e.E for e in encs)), "reads": int(sum(e.R for e in encs)),
               "encode_s": None if enc_s is None else round(enc_s, 3), "keyed_end_to_end": stats(kt), "per_key_loop": stats(lt),
               "one_key_single_scan": stats(one), "loop_over_keyed": round(med(lt) / med(kt), 2),
               "keyed_over_one_key": round(med(kt) / med(one), 2),
               "bytes_matrix": int(tot["bytes_matrix"]), "bytes_scanned": int(tot["bytes_scanned"]), "scan_ms_median": round(med(scan_ns) / 1e6, 4)}
        if name == "c":
            rec["scan_share_of_hbm"] = round(tot["bytes_scanned"] / (med(scan_ns) * 1e-9) / HBM, 3)
            rec["scan_share_of_hbm_best"] = round(tot["bytes_scanned"] / (min(scan_ns) * 1e-9) / HBM, 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

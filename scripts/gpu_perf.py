"""The perf series on synthetic histories (64 workers; 10^5 and 10^6 ops; about 10 and about 1,000 ops per one-second bucket): the whole
device call -- PerfColumns excluded, the plan, the copies, the kernels and the copies back included (`check_native`) -- against the host
statement (`perf.analyse`), and beside them the columns pass, `series_from_device`, ns_device and bytes_in.  `--trace N B` is one device
call on N ops at B ops per bucket, for `rocprofv3 --kernel-trace --stats` (the per-kernel times).  -> profiles/NOTES_perf.md"""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import jepsen_tigerbeetle_amd as pkg  # noqa: E402
from jepsen_tigerbeetle_amd.jepsen import perf as PF  # noqa: E402


def synthetic(n_ops, per_bucket, workers=64, seed=1):
    rng = random.Random(seed)
    gap = 2 * 10 ** 9 // per_bucket
    fs = ("read", "write", "cas", "add")
    h, t, busy = [], 0, [None] * workers
    while len(h) < n_ops:
        t += rng.randrange(1, gap)
        w = rng.randrange(workers)
        if busy[w] is None:
            busy[w] = rng.choice(fs)
            h.append({"type": "invoke", "f": busy[w], "value": None, "process": w, "time": t})
        else:
            r = rng.random()
            h.append({"type": "info" if r < 0.01 else ("fail" if r < 0.05 else "ok"), "f": busy[w], "value": None, "process": w, "time": t})
            busy[w] = None
    return h


def timed(fn, repeat):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    pkg.build()
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        h = synthetic(int(sys.argv[2]), int(sys.argv[3]))
        cols = PF.PerfColumns(h)
        PF.check_native(cols)
        print(json.dumps(PF.check_native(cols)["summary"]))
        return
    PF.check_native(PF.PerfColumns(synthetic(1000, 10)))          # (the first call of a process pays for the runtime's start)
    for n_ops in (10 ** 5, 10 ** 6):
        for per_bucket in (10, 1000):
            h = synthetic(n_ops, per_bucket)
            rep = 3 if n_ops <= 10 ** 5 else 1
            t_host, a = timed(lambda: PF.analyse(h), rep)
            t_cols, cols = timed(lambda: PF.PerfColumns(h), rep)
            t_dev, dev = timed(lambda: PF.check_native(cols), 3)
            t_name, ser = timed(lambda: PF.series_from_device(h, cols, dev), 1)
            t_host_series, ser_host = timed(lambda: PF.series_host(h), 1)
            s = dev["summary"]
            print(json.dumps({"n_ops": n_ops, "ops_per_bucket": per_bucket, "nb_all": s["nb_all"], "max_cell": s["max_cell"],
                              "host_analyse_s": round(t_host, 4), "host_series_s": round(t_host_series, 4), "columns_s": round(t_cols, 4),
                              "device_call_s": round(t_dev, 4), "series_from_device_s": round(t_name, 4), "ns_device": s["ns_device"],
                              "bytes_in": s["bytes_in"], "equal": ser == ser_host}), flush=True)


if __name__ == "__main__":
    main()

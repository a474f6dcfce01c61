"""Pairing event histories: the host loop (tbc_pair_events, a history a call) against the device route (tbc_pair_events_batch), on
synth.register_events histories of 10k ops (64 processes, the bench's duty cycle), at 64, 4,096 and 32,768 histories a call:
  (a) tbc_pair_events over all histories on 1 thread and on 16 threads: the loop is C on std::threads (scripts/pair_host_loop.cpp,
      compiled here with the host compiler), every thread writes its histories' ops into preallocated, already touched arrays -- what a
      C or JVM caller would get, no interpreter inside the timed region
  (b) tbc_pair_events_batch end to end (the five event columns from pageable memory, the kernels, six op columns and the descriptors
      back) and its ns_device; and the same with only the wire word and the positions asked for (what reload_events takes)
  (c) Batch.reload_events + run against Batch.reload of host-paired ops + run (the pairing of (a) is NOT in the latter)
Each the median of five runs after a warm-up.  The histories are 256 distinct ones repeated (the pairing does not care; generating 32,768
would take longer than measuring them).  -> <out>/pair_events_measure.txt (one JSON line per batch size, appended); the notes on them
are profiles/NOTES_pair_events.md.
  python scripts/gpu_pair_events.py [--sizes 64,4096,32768] [--out profiles] [--runs 5] [--no-batch]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import jepsen_tigerbeetle_amd as pkg  # noqa: E402
from jepsen_tigerbeetle_amd import _native as N, columns, core, synth  # noqa: E402
from jepsen_tigerbeetle_amd.columns import EventColumns, OpColumns  # noqa: E402

DISTINCT = 256


def say(*a):
    print(*a, flush=True)


def median_of(fn, runs):
    fn()                                                    # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


_LOOP = None


def host_loop():
    """scripts/pair_host_loop.cpp compiled with the host compiler into a temporary shared object: the loop over tbc_pair_events in C,
    on std::threads"""
    global _LOOP
    if _LOOP is None:
        here = os.path.dirname(os.path.abspath(__file__))
        so = os.path.join(tempfile.mkdtemp(prefix="pair_host_loop"), "libpair_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", os.path.join(here, "..", "include"),
                               os.path.join(here, "pair_host_loop.cpp"), "-o", so])
        _LOOP = C.CDLL(so)
        _LOOP.pair_host_loop.restype = C.c_double
        _LOOP.pair_host_loop.argtypes = [C.c_void_p, C.POINTER(N.EventBatch)] + [C.c_void_p] * 8 + [C.c_uint32]
    return _LOOP


def host_outputs(ev_off):
    """the op arrays the host loop writes, history h's ops at ev_off[h]; made once and used by every run, so that the timed runs do
    not pay for the first touch of their pages"""
    nh, n = len(ev_off) - 1, int(ev_off[-1])
    out = {k: np.zeros(max(n, 1), dt) for k, dt in (("f", np.uint8), ("a", np.int32), ("b", np.int32), ("process", np.int32), ("inv_pos", np.uint32), ("ret_pos", np.uint32))}
    return out, np.zeros(max(nh, 1), np.uint32), np.zeros(max(nh, 1), np.uint32)


def host_pairing(ev_off, ev, threads, out, n_ops, n_proc):
    """tbc_pair_events history by history on `threads` threads, the loop itself in C (no Python inside the timed region).  -> seconds"""
    i = N.EventBatch()
    i.n_hist, i.device, i.ev_off = len(ev_off) - 1, 0, columns._p(ev_off, C.c_uint64)
    i.type, i.process, i.f, i.a, i.b = (columns._p(ev.type, C.c_uint8), columns._p(ev.process, C.c_int32), columns._p(ev.f, C.c_uint8),
                                        columns._p(ev.a, C.c_int32), columns._p(ev.b, C.c_int32))
    fn = C.cast(N.lib().tbc_pair_events, C.c_void_p)
    t = host_loop().pair_host_loop(fn, C.byref(i), *[out[k].ctypes.data for k in ("f", "a", "b", "process", "inv_pos", "ret_pos")],
                                   n_ops.ctypes.data, n_proc.ctypes.data, threads)
    assert t >= 0, "tbc_pair_events refused a history"
    return t


def measure(nh, runs, with_batch):
    base = [synth.register_events(n_ops=10000, n_procs=64, seed=9000 + s, busy=0.1, n_values=4) for s in range(min(nh, DISTINCT))]
    evs = [base[h % len(base)] for h in range(nh)]
    ev_off, ev = columns.concat_events(evs)
    n = int(ev_off[-1])
    r = {"histories": nh, "events": n}
    say(f"# {nh} histories, {n} events")
    # (a)
    out, n_ops, n_proc = host_outputs(ev_off)
    for threads in (1, 16):
        ts = []
        for k in range(runs + 1):
            t = host_pairing(ev_off, ev, threads, out, n_ops, n_proc)
            ts.append(t)
            say(f"#   host, {threads} threads: {t:.3f} s")
        r[f"host_{threads}_threads_s"] = round(statistics.median(ts[1:]), 4)
    r["ops"] = int(n_ops.sum())
    # (b)
    last = {}

    def device(cols, word):
        st, got = columns.pair_events_batch_raw(ev_off, ev, ops_cap=r["ops"], columns=cols, word=word)
        N.check_status(st)
        last.update(got)

    r["device_six_columns_s"] = round(median_of(lambda: device(True, False), runs), 4)
    r["device_six_columns_ns_device"] = last["ns_device"]
    say(f"#   device, six columns: {r['device_six_columns_s']} s, kernels {last['ns_device'] / 1e6:.2f} ms")
    lo = int(ev_off[nh - 1])
    k = int(n_ops[nh - 1])
    assert last["n_ops"] == r["ops"] and last["n_bad"] == 0 and np.array_equal(last["inv_pos"][-k:], out["inv_pos"][lo:lo + k]) and np.array_equal(last["process"][-k:], out["process"][lo:lo + k])
    r["device_wire_s"] = round(median_of(lambda: device(False, True), runs), 4)
    r["device_wire_ns_device"] = last["ns_device"]
    r["bytes_in"] = last["bytes_in"]
    r["bytes_out_six_columns"] = 21 * r["ops"] + 24 * nh + 8
    r["bytes_out_wire"] = 12 * r["ops"] + 24 * nh + 8
    say(f"#   device, wire word and positions: {r['device_wire_s']} s, kernels {last['ns_device'] / 1e6:.2f} ms")
    # ... and with the event columns and the op arrays in PINNED memory (a caller that has some: the copies at the link's rate)
    try:
        import torch
        pinned = lambda m, dt: torch.empty(max(int(m), 1) * np.dtype(dt).itemsize, dtype=torch.uint8, pin_memory=True).numpy().view(dt)[:int(m)]
        pev = EventColumns(*[pinned(len(getattr(ev, c)), getattr(ev, c).dtype) for c in ("type", "process", "f", "a", "b")])
        for c in ("type", "process", "f", "a", "b"):
            getattr(pev, c)[:] = getattr(ev, c)
    except Exception as e:      # (no torch, or no pinned memory to be had: the pageable figures stand alone)
        say(f"#   no pinned memory: {e}")
        pev = None
    if pev is not None:
        def device_pinned(cols, word):
            st, got = columns.pair_events_batch_raw(ev_off, pev, ops_cap=r["ops"], columns=cols, word=word, alloc=pinned)
            N.check_status(st)
            last.update(got)

        r["device_six_columns_pinned_s"] = round(median_of(lambda: device_pinned(True, False), runs), 4)
        assert np.array_equal(last["inv_pos"][-k:], out["inv_pos"][lo:lo + k]) and np.array_equal(last["a"][-k:], out["a"][lo:lo + k])
        r["device_wire_pinned_s"] = round(median_of(lambda: device_pinned(False, True), runs), 4)
        say(f"#   device, pinned: six columns {r['device_six_columns_pinned_s']} s, wire {r['device_wire_pinned_s']} s")
        del pev
    # (c)
    last.clear()
    if with_batch:
        try:
            reload_routes(r, runs, evs, ev_off, out, n_ops, n_proc)
        except N.TbcError as e:      # (a batch of this size that the device has no room for beside the pairing's arrays: said, not hidden)
            r["reload_routes_failed"] = str(e)
            say(f"#   (c) not measured: {e}")
    return r


def reload_routes(r, runs, evs, ev_off, out, n_ops, n_proc):
    nh = len(evs)
    hists = []
    for h in range(nh):
        e0, m = int(ev_off[h]), int(n_ops[h])
        hists.append(OpColumns(*[out[c][e0:e0 + m] for c in ("f", "a", "b", "process", "inv_pos", "ret_pos")], n_events=len(evs[h]), n_process=int(n_proc[h])))
    # several histories per wavefront and a first visited set of 4 entries an op: the bench's batch (the library's default of 64 an op is
    # sixteen times the visited sets -- at 32,768 histories more than the device holds), which takes fresh inputs at every size
    opts = core.make_opts(time_limit_ms=600000, want_witness=False, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=4)
    with core.Batch(hists, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        b.run()
        say("#   batch created")
        verdicts = b.verdicts().copy()
        call = []

        def by_ops():
            b.reload(hists)
            call.append(b.reload_call_s)
            b.run()

        r["reload_ops_run_s"] = round(median_of(by_ops, runs), 4)
        r["reload_ops_call_s"] = round(statistics.median(call[1:]), 4)
        assert np.array_equal(b.verdicts(), verdicts)
        call.clear()

        def by_events():
            b.reload_events(evs)
            call.append(b.pair_call_s)
            b.run()

        r["reload_events_run_s"] = round(median_of(by_events, runs), 4)
        r["reload_events_pair_call_s"] = round(statistics.median(call[1:]), 4)
        assert np.array_equal(b.verdicts(), verdicts)
        say(f"#   reload(ops) + run {r['reload_ops_run_s']} s; reload_events + run {r['reload_events_run_s']} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,4096,32768")
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true", help="skip (c)")
    args = ap.parse_args()
    pkg.build()
    if N.lib().tbc_device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    os.makedirs(args.out, exist_ok=True)
    columns.pair_events_batch([synth.register_events(n_ops=100, n_procs=4, seed=1)])          # (the first call of a process pays for the runtime's start)
    for nh in (int(x) for x in args.sizes.split(",")):
        r = measure(nh, args.runs, not args.no_batch)
        line = json.dumps(r)
        say(line)
        with open(os.path.join(args.out, "pair_events_measure.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Event histories into a batch: the packed route (Batch.stream_events: tbc_pack_events into a pinned event slot, tbc_batch_submit_events,
the wire columns emitted on the device into the batch's stage) against the two routes that were there, on the histories and the batch of
scripts/gpu_pair_events.py case (c) -- synth.register_events histories of 10k ops, 64 processes, 256 distinct ones repeated; the bench's
batch options -- at 64, 4,096 and 32,768 histories:
  (1) stream_events + run, and its pieces: packing into the slot, the submit call, its ns_device, bytes_copied / ns_copy of input_info
  (2) host pairing on 16 threads (scripts/pair_host_loop.cpp) + reload + run
  (3) reload_events + run
Each the median of five runs after a warm-up; (3) keeps its samples, for the spread.  The measuring is done by CHILD processes, one per
(library, size), each under its own `timeout -k 10`; the driver chains them and stops at the first non-zero status.  With --parent-lib
(a libtbcheck.so built from the parent commit: a `git worktree` of it and `make -C jepsen-tigerbeetle_amd/csrc`) the two libraries
alternate -- parent, this tree, parent -- for the columns both can run, (2) and (3): the column path of the pairing kernels must not
have slowed, which is (3) of this tree's library within the parent's run-to-run spread.
-> <out>/submit_events_measure.txt (one JSON line per child, appended); the notes on them are in profiles/NOTES_pair_events.md.
  python scripts/gpu_submit_events.py [--sizes 64,4096,32768] [--out profiles] [--runs 5] [--parent-lib PATH] [--limit SECONDS]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from jepsen_tigerbeetle_amd import _native as N  # noqa: E402

NEW = ("tbc_pack_events", "tbc_pair_packed_batch", "tbc_batch_map_events", "tbc_batch_submit_events")


def say(*a):
    print(*a, flush=True)


def samples_of(fn, runs):
    fn()                                                    # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def child(args):
    """one library, one size -> one JSON line on stdout (the last line)"""
    if args.lib:                                            # another build of the library: it may lack what this tree adds
        N.LIB_PATH = os.path.abspath(args.lib)
        probe = C.CDLL(N.LIB_PATH)
        for name in NEW:
            if not hasattr(probe, name):
                N.SYMBOLS.pop(name, None)
    from jepsen_tigerbeetle_amd import columns, core, synth
    from jepsen_tigerbeetle_amd.columns import OpColumns
    import gpu_pair_events as G
    lib = N.lib()
    if lib.tbc_device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    has_new = "tbc_batch_submit_events" in N.SYMBOLS
    nh, runs = args.size, args.runs
    med = lambda xs: round(statistics.median(xs), 4)
    base = [synth.register_events(n_ops=10000, n_procs=64, seed=9000 + s, busy=0.1, n_values=4) for s in range(min(nh, G.DISTINCT))]
    evs = [base[h % len(base)] for h in range(nh)]
    ev_off, ev = columns.concat_events(evs)
    r = {"library": args.label, "histories": nh, "events": int(ev_off[-1])}
    say(f"# {args.label}: {nh} histories, {r['events']} events")
    # (2), its host part
    out, n_ops, n_proc = G.host_outputs(ev_off)
    ts = [G.host_pairing(ev_off, ev, 16, out, n_ops, n_proc) for _ in range(runs + 1)]
    r["host_16_threads_s"] = med(ts[1:])
    r["ops"] = int(n_ops.sum())
    del ev
    hists = []
    for h in range(nh):
        e0, m = int(ev_off[h]), int(n_ops[h])
        hists.append(OpColumns(*[out[c][e0:e0 + m] for c in ("f", "a", "b", "process", "inv_pos", "ret_pos")], n_events=len(evs[h]), n_process=int(n_proc[h])))
    opts = core.make_opts(time_limit_ms=600000, want_witness=False, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=4)
    with core.Batch(hists, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        b.run()
        verdicts = b.verdicts().copy()
        say("#   batch created")

        def by_ops():
            b.reload(hists)
            b.run()

        r["reload_ops_run_s"] = med(samples_of(by_ops, runs))
        r["host_pairing_reload_run_s"] = round(r["host_16_threads_s"] + r["reload_ops_run_s"], 4)
        assert np.array_equal(b.verdicts(), verdicts)
        say(f"#   (2) host pairing {r['host_16_threads_s']} s + reload + run {r['reload_ops_run_s']} s")

        def by_events():
            b.reload_events(evs)
            b.run()

        ts = samples_of(by_events, runs)
        r["reload_events_run_s"], r["reload_events_run_samples"] = med(ts), [round(t, 4) for t in ts]
        assert np.array_equal(b.verdicts(), verdicts)
        say(f"#   (3) reload_events + run {r['reload_events_run_s']} s {r['reload_events_run_samples']}")
        if has_new:
            pieces = {"pack_s": [], "submit_s": [], "ns_device": [], "ns_copy": []}

            def by_stream():
                b.stream_events(evs)
                b.run()
                info = b.input_info()
                pieces["pack_s"].append(b.pack_s), pieces["submit_s"].append(b.submit_s), pieces["ns_device"].append(b.events_report["ns_device"])
                pieces["ns_copy"].append(info["ns_copy"])
                r["stream_bytes_copied"] = info["bytes_copied"]

            t0 = time.perf_counter()
            b.map_events(0), b.map_events(1)
            r["map_events_first_s"] = round(time.perf_counter() - t0, 3)          # (once a batch: the pinned slots and the device arena)
            ts = samples_of(by_stream, runs)
            r["stream_events_run_s"], r["stream_events_run_samples"] = med(ts), [round(t, 4) for t in ts]
            for k, v in pieces.items():
                r["stream_" + k] = med(v[1:]) if k.endswith("_s") else int(statistics.median(v[1:]))
            r["device_bytes"] = int(lib.tbc_batch_device_bytes(b._h))
            assert np.array_equal(b.verdicts(), verdicts)
            say(f"#   (1) stream_events + run {r['stream_events_run_s']} s: pack {r['stream_pack_s']} s, submit {r['stream_submit_s']} s, "
                f"kernels {r['stream_ns_device'] / 1e6:.2f} ms, {r['stream_bytes_copied']} B in {r['stream_ns_copy'] / 1e6:.2f} ms")
    say(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,4096,32768")
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtbcheck.so built from the parent commit")
    ap.add_argument("--limit", type=int, default=900, help="seconds a child may take")
    ap.add_argument("--size", type=int, default=0, help="(a child) the one size to measure")
    ap.add_argument("--lib", default=None, help="(a child) the library to load instead of the tree's")
    ap.add_argument("--label", default="tree", help="(a child) what the line calls its library")
    args = ap.parse_args()
    if args.size:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    for nh in (int(x) for x in args.sizes.split(",")):
        turns = [("parent", args.parent_lib), ("tree", None), ("parent", args.parent_lib)] if args.parent_lib else [("tree", None)]
        for label, lib in turns:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--size", str(nh), "--runs", str(args.runs), "--label", label]
            if lib:
                cmd += ["--lib", lib]
            last = ""
            with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as p:
                for line in p.stdout:                       # (passed on as it comes)
                    say(line.rstrip("\n"))
                    last = line if line.strip() else last
            if p.returncode != 0:                           # (a fault, a hang, a failed assertion: nothing more is started)
                raise SystemExit(f"the child for {label}, {nh} histories ended with status {p.returncode}: stopping")
            with open(os.path.join(args.out, "submit_events_measure.txt"), "a") as f:
                f.write(last.strip() + "\n")


if __name__ == "__main__":
    main()

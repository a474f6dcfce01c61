"""set-full from op columns (tbc_setfull_keys_create_ops) against the host encoder (`Encoded` + tbc_setfull_keys_create), this commit
alternated with its parent: one process per build and shape, the raw lines kept (as profiles/NOTES_setfull_merge.md).

Shapes: scripts/gpu_setfull_keys.py's (a) 5 keys x 10k ops and (b) 256 keys x 2k ops, as histories.  (The bench's single
262,144 x 32,768 key is left out: its raw read values would be about 34 GB.)

Per process one JSON line:
  both builds   encoded_s            `Encoded` over all keys
                check_keys_s         sf.check_keys as a whole call (encoding included)
                create_rows_ms       tbc_setfull_keys_create given the ready compact form + destroy, bare C calls
                scan_rows_ms         ns_scan of that object, run after run
  this commit   columns_s            `OpColumns.of_keys`
                check_columns_s      sf.check_keys_columns as a whole call (== check_keys' maps, asserted)
                create_ops_ms        tbc_setfull_keys_create_ops + destroy, bare C calls
                encode_ms, value_bytes   ns_encode and the bytes of read values it went through
                scan_ops_ms          ns_scan of the object made from ops: to lie inside scan_rows_ms's own min - max band

  python scripts/gpu_setfull_ops.py --parent-lib PATH [--rounds 2] [--shapes ab]      (PATH: the parent commit's libtbcheck.so)
  python scripts/gpu_setfull_ops.py --child a --tag new                               one process, one line"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW = ("tbc_setfull_keys_create_ops", "tbc_setfull_keys_shape", "tbc_setfull_keys_encoding")


def histories(name):
    from helpers import set_history
    if name == "a":
        return {k: set_history(10_000, 10, 300 + k, busy=0.3, info=0.02) for k in range(5)}
    return {k: set_history(2_000, 6, 500 + k, busy=0.3, info=0.02) for k in range(256)}


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def child(name, tag, reps):
    from jepsen_tigerbeetle_amd import _native as N
    if tag == "parent":                                   # (the parent's library lacks the new entry points: do not bind them)
        for s in NEW:
            N.SYMBOLS.pop(s, None)
    from jepsen_tigerbeetle_amd.jepsen import set_full as sf
    hists = histories(name)
    r3 = lambda xs: [round(x, 4) for x in xs]
    rec = {"what": name, "lib": tag, "keys": len(hists), "ops": sum(len(h) for h in hists.values())}
    enc_s, encs = timed(lambda: [sf.Encoded(h) for h in hists.values()])
    rec["encoded_s"] = round(enc_s, 3)
    whole = [timed(lambda: sf.check_keys(hists, True)) for _ in range(2)]
    rec["check_keys_s"] = r3([t for t, _ in whole])

    def bare_rows():
        with sf.KeyedScan(encs):
            pass
    bare_rows()
    rec["create_rows_ms"] = r3([1e3 * timed(bare_rows)[0] for _ in range(reps)])
    with sf.KeyedScan(encs) as ks:
        ks.run()
        rec["scan_rows_ms"] = r3([ks.run()[1]["ns_scan"] / 1e6 for _ in range(reps)])
    if tag != "parent":
        col_s, cols = timed(lambda: sf.OpColumns.of_keys(hists))
        rec["columns_s"] = round(col_s, 3)
        wc = [timed(lambda: sf.check_keys_columns(hists, True)) for _ in range(2)]
        rec["check_columns_s"] = r3([t for t, _ in wc])
        assert wc[0][1] == whole[0][1], "check_keys_columns differs from check_keys"

        def bare_ops():
            with sf.KeyedScan.from_ops(cols):
                pass
        bare_ops()
        rec["create_ops_ms"] = r3([1e3 * timed(bare_ops)[0] for _ in range(reps)])
        with sf.KeyedScan.from_ops(cols) as ko:
            rec["encode_ms"] = round(ko.encoding()["ns_encode"] / 1e6, 4)
            rec["value_bytes"] = int(len(cols.vals)) * 8
            ko.run()
            rec["scan_ops_ms"] = r3([ko.run()[1]["ns_scan"] / 1e6 for _ in range(reps)])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shapes", default="ab")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--child", default=None)
    ap.add_argument("--tag", default="new")
    ap.add_argument("--limit", type=int, default=240, help="seconds one process may take")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.tag, args.reps)
        return
    builds = ([("parent", args.parent_lib)] if args.parent_lib else []) + [("new", None)]
    lines = []
    for _ in range(args.rounds):                         # alternated, so that drift hits both alike
        for name in args.shapes:
            for tag, lib in builds:
                env = dict(os.environ)
                env.pop("TBC_LIB_PATH", None)
                if lib:
                    env["TBC_LIB_PATH"] = os.path.abspath(lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--tag", tag, "--reps", str(args.reps)], env=env,
                                   capture_output=True, text=True, timeout=args.limit)
                if p.returncode != 0:                    # (a process that ended badly ends the run: nothing more is started on the GPU)
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(p.returncode if p.returncode > 0 else 1)
                line = p.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                lines.append(json.loads(line))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for name in args.shapes:
        new = [r for r in lines if r["what"] == name and r["lib"] == "new"]
        par = [r for r in lines if r["what"] == name and r["lib"] == "parent"] or new
        rows, ops = [x for r in new for x in r["scan_rows_ms"]], [x for r in new for x in r["scan_ops_ms"]]
        print(json.dumps({"summary": name,
                          "parent_check_keys_s": med([x for r in par for x in r["check_keys_s"]]), "parent_encoded_s": med([r["encoded_s"] for r in par]),
                          "check_columns_s": med([x for r in new for x in r["check_columns_s"]]), "columns_s": med([r["columns_s"] for r in new]),
                          "create_rows_ms": med([x for r in new for x in r["create_rows_ms"]]), "create_ops_ms": med([x for r in new for x in r["create_ops_ms"]]),
                          "parent_create_rows_ms": med([x for r in par for x in r["create_rows_ms"]]),
                          "encode_ms": med([r["encode_ms"] for r in new]), "value_bytes": new[0]["value_bytes"],
                          "scan_rows_band_ms": [min(rows), max(rows)], "scan_ops_median_ms": med(ops),
                          "scan_ops_inside_band": min(rows) <= med(ops) <= max(rows)}), flush=True)


if __name__ == "__main__":
    main()

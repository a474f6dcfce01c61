"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The front walk in the form the kernel launches it (walk::walk_run, csrc/open_walk_impl.h: a
wavefront takes a run of consecutive chunks of one history and carries the slot cursors from chunk to chunk) under the wavefront
emulator: builds tests/emu/_build/libemu_walk_runs.so with g++ from emu_walk_runs.cpp and runs it through ctypes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "jepsen-tigerbeetle_amd", "csrc")
_SO = os.path.join(_HERE, "_build", "libemu_walk_runs.so")
_SRCS = [os.path.join(_HERE, "emu_walk_runs.cpp"), os.path.join(_HERE, "walk_harness.h"), os.path.join(_HERE, "wave_env_emu.h"), os.path.join(_HERE, "host_tables.h"),
         os.path.join(_CSRC, "open_walk_impl.h"), os.path.join(_CSRC, "tbc_internal.h"), os.path.join(_CSRC, "wave_env.h")]
_FLAGS = ["-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", _HERE, "-I", _CSRC]
_LIB = None


def build(force=False):
    if force or not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-fPIC", "-shared"] + _FLAGS + ["-o", _SO, _SRCS[0]])
    return _SO


def build_program(out, sanitize=True):
    """the harness as a program of its own (reads a batch dump() wrote): what a sanitizer run uses -- nothing is loaded into python"""
    subprocess.check_call(["g++", "-O1", "-DEMU_WALK_RUNS_MAIN"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
                          + _FLAGS + ["-o", out, _SRCS[0]])
    return out


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.emu_walk_runs_check.restype = C.c_int
        _LIB.emu_walk_run_length.restype = C.c_uint32
    return _LIB


def run_length():
    """the kernel's kWalkRun"""
    return int(_lib().emu_walk_run_length())


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _columns(hists):
    ds = [h if isinstance(h, dict) else h.as_dict() for h in hists]
    nh = len(ds)
    op_off = np.zeros(nh + 1, np.uint64)
    for i, d in enumerate(ds):
        op_off[i + 1] = op_off[i] + len(d["f"])
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(d[k], dt) for d in ds]), dt)
    npr = np.array([int(d["n_process"]) for d in ds], np.uint32)
    assert int(npr.max()) <= 64
    return nh, op_off, npr, cat("f", np.uint8), cat("a", np.int32), cat("b", np.int32), cat("process", np.int32), cat("inv_pos", np.uint32), cat("ret_pos", np.uint32)


def _flags(twin, look, branch, front, by_ret):
    return ((1 if twin else 0) | (2 if look else 0) | (4 if branch else 0) | {"plain": 0, "wide": 8, "compact": 24}[front]
            | ((int(by_ret) << 16) if int(by_ret) >= 16 else 128 if by_ret == 2 else 64 if by_ret else 0))


def expected_counts(hists, run):
    """(runs that have a front, chunks that have fronts) from the histories themselves: a front per completed call"""
    runs = chunks = 0
    for h in hists:
        d = h if isinstance(h, dict) else h.as_dict()
        n_ret = int((np.asarray(d["ret_pos"], np.uint32) != 0xFFFFFFFF).sum())
        c = (n_ret + 63) // 64
        chunks += c
        runs += (c + run - 1) // run
    return runs, chunks


WHAT = {1: "lst", 2: "twn", 3: "rdm", 4: "look word 0", 5: "look mask", 6: "tmp", 9: "bad input"}
COUNT_NAMES = ("searches", "carried", "mismatches", "runs", "chunks")


def call_check(fn, hists, vpad, flags, run=None):
    """One of the harness's checks (emu_walk_check: run=None, it takes neither run nor counts; emu_walk_runs_check,
    emu_walk_sparse_count_check) on these histories.  Returns (None or (what, history, front, index, got, want), counts)."""
    nh, op_off, npr, f, a, b, pr, inv, ret = _columns(hists)
    diag = np.zeros(8, np.uint64)
    cnt = np.zeros(8, np.uint64)
    fn.restype = C.c_int
    rc = fn(C.c_uint32(nh), _p(op_off, C.c_uint64), _p(npr, C.c_uint32), _p(f, C.c_uint8), _p(a, C.c_int32), _p(b, C.c_int32),
            _p(pr, C.c_int32), _p(inv, C.c_uint32), _p(ret, C.c_uint32), C.c_uint32(vpad), C.c_uint32(flags),
            *(() if run is None else (C.c_uint32(run),)), _p(diag, C.c_uint64), *(() if run is None else (_p(cnt, C.c_uint64),)))
    counts = dict(zip(COUNT_NAMES, (int(x) for x in cnt[:5])))
    if rc == 0:
        return None, counts
    return (WHAT.get(rc, str(rc)), int(diag[0]), int(diag[1]), int(diag[2]), hex(int(diag[3])), hex(int(diag[4]))), counts


def walk_runs_check(hists, vpad, run=0, twin=True, look=True, branch=False, front="plain", by_ret=0):
    """Run walk_run (run chunks a wavefront: 0 = the kernel's kWalkRun, or 2, 3) on these histories and compare every word it writes with
    the host-built tables.  Returns (None or (what, history, front, index, got, want), counts) with counts = dict(searches, carried,
    mismatches, runs, chunks): chunks that searched / took carried cursors, slot lanes whose carried cursor was not the searched one, and
    the harness's own count of (history, run) pairs and chunks that have a front."""
    return call_check(_lib().emu_walk_runs_check, hists, vpad, _flags(twin, look, branch, front, by_ret), run)


def dump(path, hists, vpad, run=0, twin=True, look=True, branch=False, front="plain", by_ret=0):
    """the batch as a file for the stand-alone program (build_program)"""
    nh, op_off, npr, f, a, b, pr, inv, ret = _columns(hists)
    with open(path, "wb") as fp:
        for arr in (np.array([nh, vpad, _flags(twin, look, branch, front, by_ret), run], np.uint32), op_off, npr, f, a, b, pr, inv, ret):
            raw = arr.tobytes()
            fp.write(raw + b"\0" * (-len(raw) % 8))

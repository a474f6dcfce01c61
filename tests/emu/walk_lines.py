"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The sparse form's list stores with lane = entry (csrc/open_walk_impl.h, sparse_lists) under the
wavefront emulator: builds tests/emu/_build/libemu_walk_lines*.so with g++ from emu_walk_lines.cpp (the sparse-form harness plus a second,
chunk-by-chunk run that holds the form's counts against the host-built tables per chunk) and runs it through ctypes.  A build can carry one
planted mutation of the kernel body."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import walk_runs, walk_sparse

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu_walk_lines.cpp")
_SRCS = [_SRC] + walk_sparse._SRCS
MUTATIONS = {
    "rank_off_by_one": "-DTBC_WALK_RANK_OFF_BY_ONE",          # an entry's rank within its front one too high
    "front_le": "-DTBC_WALK_FRONT_LE",                        # start <= e0 for start < e0: a front whose first entry is a pass's first is not found there
}
LINE_NAMES = ("chunks", "sparse", "passes", "passes_expected", "entries", "entries_expected", "chunks_off", "fronts_apart", "no_candidate", "second_set")
_LIBS = {}


def _so(mutation):
    return os.path.join(_HERE, "_build", "libemu_walk_lines%s.so" % ("_" + mutation if mutation else ""))


def build(mutation=None, force=False):
    so = _so(mutation)
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _SRCS):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-fPIC", "-shared"] + walk_runs._FLAGS + ([MUTATIONS[mutation]] if mutation else []) + ["-o", so, _SRC])
    return so


def build_program(out, sanitize=True):
    """the harness as a program of its own (reads a batch dump() wrote): what a sanitizer run uses -- nothing is loaded into python"""
    subprocess.check_call(["g++", "-O1", "-DEMU_WALK_LINES_MAIN"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
                          + walk_runs._FLAGS + ["-o", out, _SRC])
    return out


def dump(path, hists, vpad=8, count_form=False, **kw):
    """the batch as a file for the stand-alone program"""
    walk_runs.dump(path, hists, vpad, run=256 if count_form else 0, **kw)


def check(hists, vpad=8, twin=True, look=True, branch=False, front="plain", by_ret=0, mutation=None, count_form=False):
    """walk_run on these histories, then every chunk once more from nothing: every word against the host-built tables both times.  Returns
    (None or (what, history, front, index, got, want), counts, chunk_entries, chunk_sparse): counts = the run form's (walk_runs.COUNT_NAMES)
    plus LINE_NAMES; chunk_entries / chunk_sparse: per chunk that has fronts, history by history, its list entries by off[] and whether it
    took the sparse form."""
    lib = C.CDLL(build(mutation)) if mutation not in _LIBS else _LIBS[mutation]
    _LIBS[mutation] = lib
    lib.emu_walk_lines_check.restype = C.c_int
    nh, op_off, npr, f, a, b, pr, inv, ret = walk_runs._columns(hists)
    diag, cnt, lines = np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    cap = int(op_off[-1]) // 64 + nh + 1
    ce, cs = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    p = walk_runs._p
    rc = lib.emu_walk_lines_check(C.c_uint32(nh), p(op_off, C.c_uint64), p(npr, C.c_uint32), p(f, C.c_uint8), p(a, C.c_int32), p(b, C.c_int32), p(pr, C.c_int32),
                                  p(inv, C.c_uint32), p(ret, C.c_uint32), C.c_uint32(vpad), C.c_uint32(walk_runs._flags(twin, look, branch, front, by_ret)),
                                  C.c_uint32(1 if count_form else 0), p(diag, C.c_uint64), p(cnt, C.c_uint64), p(lines, C.c_uint64), p(ce, C.c_uint32), p(cs, C.c_uint8),
                                  C.c_uint32(cap))
    counts = dict(zip(walk_runs.COUNT_NAMES, (int(x) for x in cnt[:5])))
    counts.update(zip(LINE_NAMES, (int(x) for x in lines[:len(LINE_NAMES)])))
    n = counts["chunks"] if rc == 0 else 0
    bad = None if rc == 0 else (("chunk form: " if rc & 16 else "") + walk_runs.WHAT.get(rc & 15, str(rc)), int(diag[0]), int(diag[1]), int(diag[2]), hex(int(diag[3])), hex(int(diag[4])))
    return bad, counts, [int(x) for x in ce[:n]], [int(x) for x in cs[:n]]

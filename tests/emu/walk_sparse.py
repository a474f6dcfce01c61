"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The sparse form of the front walk's phase C (csrc/open_walk_impl.h) under the wavefront
emulator: builds tests/emu/_build/libemu_walk_sparse*.so with g++ from emu_walk_sparse.cpp (the run-form harness plus the form's schedule
counts and a switch to the dense loop) and runs it through ctypes.  A build can carry one planted mutation of the kernel body."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import walk_runs

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu_walk_sparse.cpp")
_SRCS = [_SRC] + walk_runs._SRCS
MUTATIONS = {
    "off_at_ret": "-DTBC_WALK_OFF_AFTER=0u",                 # a call's bit goes OFF at ret instead of ret + 1
    "twin_le": "-DTBC_WALK_TWIN_LE",                          # ret_u <= ret_c
    "no_self_exclusion": "-DTBC_WALK_NO_SELF_EXCLUSION",      # the completing call counts as a producer of what it needs
}
STAT_NAMES = ("sparse", "dense", "emit_trips", "twin_steps", "rounds", "twin_find", "nc_le64", "nc_mid", "nc_more", "find_wave", "chain_wave")
_LIBS = {}


def _so(mutation):
    return os.path.join(_HERE, "_build", "libemu_walk_sparse%s.so" % ("_" + mutation if mutation else ""))


def build(mutation=None, force=False):
    so = _so(mutation)
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _SRCS):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-fPIC", "-shared"] + walk_runs._FLAGS + ([MUTATIONS[mutation]] if mutation else []) + ["-o", so, _SRC])
    return so


def build_program(out, sanitize=True):
    """the harness as a program of its own (reads a batch walk_runs.dump() wrote): what a sanitizer run uses -- nothing is loaded into python"""
    subprocess.check_call(["g++", "-O1", "-DEMU_WALK_RUNS_MAIN"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
                          + walk_runs._FLAGS + ["-o", out, _SRC])
    return out


def _lib(mutation=None):
    if mutation not in _LIBS:
        lib = C.CDLL(build(mutation))
        lib.emu_walk_runs_check.restype = C.c_int
        lib.emu_walk_sparse_count_check.restype = C.c_int
        _LIBS[mutation] = lib
    return _LIBS[mutation]


def check(hists, vpad, run=0, twin=True, look=True, branch=False, front="plain", by_ret=0, mutation=None, dense=False, count_form=False):
    """walk_run on these histories, every word against the host-built tables.  Returns (None or (what, history, front, index, got, want),
    counts): walk_runs.walk_runs_check's counts plus the sparse form's (STAT_NAMES).  dense: every chunk takes the dense loop.  count_form: the histories as the count form
    lays them out (live calls on re-used slots, crashed calls on none); run must be 0 there."""
    lib = _lib(mutation)
    st = np.zeros(16, np.uint64)
    lib.emu_walk_force_dense(C.c_int(1 if dense else 0))
    lib.emu_walk_sparse_stats(walk_runs._p(st, C.c_uint64), C.c_int(1))
    try:
        err, counts = walk_runs.call_check(lib.emu_walk_sparse_count_check if count_form else lib.emu_walk_runs_check, hists, vpad,
                                           walk_runs._flags(twin, look, branch, front, by_ret), run)
    finally:
        lib.emu_walk_force_dense(C.c_int(0))
    lib.emu_walk_sparse_stats(walk_runs._p(st, C.c_uint64), C.c_int(1))
    counts.update(zip(STAT_NAMES, (int(x) for x in st[:len(STAT_NAMES)])))
    return err, counts

"""The deciding kernels of tbc_setfull_results (csrc/set_full_results.h, the file hipcc compiles into libtbcheck.so) on the CPU under the
wavefront / workgroup emulator of tests/emu (tests/emu/emu_setfull_results.cpp launches them in the library's order), against the
numpy model of tests/test_set_full_results.py over the numpy reduction's three indices: outcome, both latencies, counts, verdict,
quantiles and worst stale, exactly, under several seeded interleavings of the wavefronts.  Test infrastructure only: the product has no
CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.columns import _p
from jepsen_tigerbeetle_amd.jepsen import set_full as sf
from test_set_full_keys import _dense_states, _synthetic_key
from test_set_full_results import FAMILIES, _all_stable_key, _assert_same, _check_family_is_adequate, _family_times, _late_reads_key, _n_ops, np_decide

NONE = N.NO_OP


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_sfr") / "libemu_sfr.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_setfull_results.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_setfull_results.restype = C.c_int
    return lib


def _run(lib, states, times, unit, lin, seed):
    """states: per key (known, lp, la); times: per key an int64 array, or None -> per key what KeyedScan.results gives"""
    Es = np.array([len(s[0]) for s in states], np.uint32)
    n = max(1, int(Es.sum()))
    cat = lambda i: np.ascontiguousarray(np.concatenate([np.asarray(s[i], np.uint32) for s in states] + [np.zeros(1, np.uint32)]))
    known, lp, la = cat(0), cat(1), cat(2)
    outcome, slat, llat = np.full(n, 9, np.uint8), np.full(n, -7, np.int64), np.full(n, -7, np.int64)
    summary = (N.SetFullKeySummary * len(states))()
    op_time = off = None
    if times is not None:
        off = np.concatenate([[0], np.cumsum([len(t) for t in times])]).astype(np.uint64)
        op_time = np.ascontiguousarray(np.concatenate(list(times) + [np.zeros(1, np.int64)]), np.int64)
    rc = lib.emu_setfull_results(C.c_uint32(len(states)), _p(Es, C.c_uint32), _p(known, C.c_uint32), _p(lp, C.c_uint32), _p(la, C.c_uint32),
                                 None if op_time is None else _p(op_time, C.c_int64), None if off is None else _p(off, C.c_uint64),
                                 C.c_uint64(unit), C.c_uint32(N.SETFULL_F_LINEARIZABLE if lin else 0), _p(outcome, C.c_uint8),
                                 _p(slat, C.c_int64), _p(llat, C.c_int64), summary, C.c_uint64(seed))
    assert rc == 0
    cut = np.concatenate([[0], np.cumsum(Es, dtype=np.int64)])
    return [{"outcome": outcome[a:b], "stable_latency": slat[a:b], "lost_latency": llat[a:b], "summary": sf.summary_dict(summary[k])}
            for k, (a, b) in enumerate(zip(cut[:-1], cut[1:]))]


def _states(a):
    d = _dense_states(a)
    return d["known"], d["last_present"], d["last_absent"]


@pytest.mark.parametrize("family", FAMILIES)
def test_kernels_equal_numpy_on_edge_shapes_and_a_key_of_three_workgroups(emu, family):
    """Keys of 0 .. 257 elements (an empty one first, in the middle and last) and one of 5,000 -- three workgroups counting into one
    key's histograms -- in one launch sequence, every latency family, two interleavings."""
    arrs = [_synthetic_key(E, R, 31 * E + R) for E, R in ((0, 3), (1, 1), (31, 64), (33, 65), (64, 1), (0, 0), (65, 64), (255, 65), (257, 64))]
    arrs += [_late_reads_key(5000, 8, 4, unread=40), _synthetic_key(0, 2, 9)]
    states = [_states(a) for a in arrs]
    cols = [_family_times(family, _n_ops(a), 5 + i) for i, a in enumerate(arrs)]
    unit = cols[0][1]
    wants = [np_decide(*s, t, unit, True) for s, (t, _) in zip(states, cols)]
    _check_family_is_adequate(family, wants)
    for seed in (1, 2):
        got = _run(emu, states, None if family == "none" else [t for t, _ in cols], unit, True, seed)
        for i, (g, w) in enumerate(zip(got, wants)):
            _assert_same(g, w, (family, i, arrs[i].E, seed))


@pytest.mark.parametrize("n", (1, 2, 20, 100, 101))
def test_quantile_ranks(emu, n):
    rng = np.random.default_rng(n)
    lat = rng.permutation(np.arange(n) * 3 + (rng.integers(0, 2 ** 40) if n > 2 else 0))
    a, t = _all_stable_key(lat)
    st = (a.add_ok, np.full(a.E, a.read_invoke[0], np.uint32), np.full(a.E, NONE, np.uint32))
    got = _run(emu, [st], [t], 1, False, n)[0]
    _assert_same(got, np_decide(*st, t, 1, False), n)
    assert got["summary"]["stable_count"] == n and got["summary"]["valid"] is True


def test_worst_stale_and_verdicts(emu):
    lats = ([0, 5, 0, 9, 5, 0, 2], [3, 0, 8, 8, 1, 0, 6, 2, 7, 0, 4], [7, 9, 0, 7, 3, 9, 7, 9, 1, 9, 7, 9, 7, 0, 9, 3, 7], [0] * 40,
            [4] * 3000)                              # 3,000 ties for eight places across two workgroups: the lowest numbers win
    keys = [_all_stable_key(x) for x in lats]
    states = [(a.add_ok, np.full(a.E, a.read_invoke[0], np.uint32), np.full(a.E, NONE, np.uint32)) for a, _ in keys]
    states.append((np.array([1, NONE, 5], np.uint32), np.full(3, NONE, np.uint32), np.array([NONE, 9, NONE], np.uint32)))      # nothing stable
    states.append((np.array([1, 3], np.uint32), np.array([4, 2], np.uint32), np.array([NONE, 6], np.uint32)))                  # one lost
    times = [t for _, t in keys] + [np.zeros(10, np.int64), np.arange(10, dtype=np.int64)]
    for lin in (True, False):
        got = _run(emu, states, times, 1, lin, 3)
        for i, (g, s, t) in enumerate(zip(got, states, times)):
            _assert_same(g, np_decide(*s, t, 1, lin), (i, lin))
        assert [g["summary"]["valid"] for g in got] == [not lin, not lin, not lin, True, not lin, "unknown", False]
    assert [w["element"] for w in got[2]["summary"]["worst"]] == [1, 5, 7, 9, 11, 14, 0, 3]
    assert [w["element"] for w in got[4]["summary"]["worst"]] == list(range(8))

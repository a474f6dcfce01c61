"""tbc_ledger_realtime on the CPU: the host plan (csrc/ledger_rt_plan.h) and the kernels of csrc/ledger_rt_kernels.h -- the file hipcc
compiles into libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_ledger_rt.cpp lays the arena out and
runs the kernels in the library's launch order, every grid capped at 3 workgroups so that the grid strides run, a chunk one wavefront's
64 entries -- and once several wavefronts' worth --), against realtime_numpy of jepsen/ledger.py: every output array and every summary field, exactly, under two seeded
interleavings of the wavefronts, on the shape cases of tests/test_ledger_realtime_gpu.py.  Test infrastructure only: the product has no
CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ledger_realtime_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

SEEDS = (1, 2)
CASES = G.shape_cases()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_rt") / "libemu_rt.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_ledger_rt.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_rt_check.restype = C.c_int
    lib.emu_rt_error.restype = C.c_char_p
    return lib


def emu_check(lib, history, opts, seed, grid=3, chunks_cap=0):
    accounts, init, apply_ok = L._rt_opts(None, opts)
    cols = L.LedgerColumns(history)

    def call(s, out):
        assert lib.emu_rt_check(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed), C.c_uint32(chunks_cap)) == 0, lib.emu_rt_error().decode()

    return cols, L.check_realtime_native(cols, accounts, init, apply_ok, call=call)


def assert_same(got, want, tag):
    for k in ("bits", "miss", "lo", "hi", "floor"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")} == want["summary"], tag


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_numpy_statement(emu, case):
    h, o = case["history"], case["opts"]
    want = L.realtime_numpy(h, o)
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert want["summary"][k] == v, (case["name"], k)
    cols = L.LedgerColumns(h)
    s, keep = L.ledger_rt_in(cols, *L._rt_opts(None, o))
    shape = (C.c_uint64 * 14)()
    assert emu.emu_rt_shape(C.byref(s), shape) == 0
    assert [int(shape[4 * k + 3]) for k in range(3)] == [64, 64, 64]          # a chunk is one wavefront
    assert int(shape[12]) == len(cols.read_ops) and int(shape[13]) == 2 * len(o["accounts"])
    for seed in SEEDS:
        cols, got = emu_check(emu, h, o, seed)
        assert_same(got, want, (case["name"], seed))
    accounts, init, apply_ok = L._rt_opts(None, o)
    assert L.realtime_result_map(h, cols, got, accounts, init, apply_ok) == L._rt_map(h, want["summary"], accounts, init, apply_ok)


def test_list_lengths_around_a_chunk(emu):
    """account 1's credit list of 63, 64, 65 entries spans exactly one chunk +- 1: the plan cuts the stream where the case says"""
    for n in (63, 64, 65):
        h, o = next((c["history"], c["opts"]) for c in CASES if c["name"] == f"list-of-{n}")
        s, keep = L.ledger_rt_in(L.LedgerColumns(h), *L._rt_opts(None, o))
        shape = (C.c_uint64 * 14)()
        assert emu.emu_rt_shape(C.byref(s), shape) == 0
        assert int(shape[5]) == n + 3 and int(shape[6]) == (2 * (n + 3) + 63) // 64
    for n, chunks in ((31, 1), (32, 1), (33, 2)):                             # ... and a stream of 62, 64, 66 entries is one chunk, one, two
        h, o = next((c["history"], c["opts"]) for c in CASES if c["name"] == f"chunk-of-{2 * n}-entries")
        s, keep = L.ledger_rt_in(L.LedgerColumns(h), *L._rt_opts(None, o))
        shape = (C.c_uint64 * 14)()
        assert emu.emu_rt_shape(C.byref(s), shape) == 0
        assert (int(shape[1]), int(shape[2]), int(shape[5]), int(shape[6])) == (n, chunks, n, chunks)


def test_chunks_of_several_wavefronts(emu):
    """one or two chunks per stream, so a chunk takes several steps of 64 entries: the carried (count, value) of a class goes from step to
    step through the chunk's own row (rt_scan_kernel's atomics with return), and from the first chunk to the second through the carry"""
    for name in ("eight-accounts", "65-accounts", "list-of-65", "straddle", "all-on-one-account", "reverse-completion", "planted-all"):
        case = next(c for c in CASES if c["name"] == name)
        want = L.realtime_numpy(case["history"], case["opts"])
        assert 2 * max(want["summary"]["n_checked"], want["summary"]["n_possible"]) > 64        # (a stream of more than one wavefront's worth of entries)
        for seed, cap in zip(SEEDS, (1, 2)):                                   # one chunk for the whole stream; two chunks
            _, got = emu_check(emu, case["history"], case["opts"], seed, grid=2, chunks_cap=cap)
            assert_same(got, want, (name, seed, cap))


def test_no_accounts_at_all(emu):
    """what only a direct caller of the C entry can ask: no account, so every side names none (and is counted), nothing is checked, and an
    amount out of range is still found"""
    h, o, _ = G.concurrent_ledger(5, ops=40, fail=0.0)
    cols = L.LedgerColumns(h)
    want = L.realtime_numpy_columns(cols, [], {}, True)
    assert want["summary"]["foreign_sides"] > 0 and want["summary"]["n_checked"] == 0 and (want["hi"] == L._I64_MIN).all()

    def call(s, out):
        assert emu.emu_rt_check(C.byref(s), C.byref(out), C.c_uint32(2), C.c_uint64(1), C.c_uint32(0)) == 0, emu.emu_rt_error().decode()

    assert_same(L.check_realtime_native(cols, [], {}, True, call=call), want, "no accounts")
    t = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))[0]
    cols.mop_c[int(cols.mop_off[t])] = -1
    s, keep = L.ledger_rt_in(cols, [], {}, True)
    out = N.LedgerRtOut()
    assert emu.emu_rt_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0)) == N.ERR_UNSUPPORTED and out.summary.bad_amounts == 1


def test_random_concurrent_ledgers_and_ok_transfers_apply_false(emu):
    for seed, plant in enumerate([(), ("stale",), ("future", "regressed"), G.ANOMALIES]):
        h, o, planted = G.concurrent_ledger(40 + seed, workers=6, ops=120, plant=plant)
        assert set(planted) == set(plant)
        for apply_ok in (True, False):
            o2 = dict(o, **{"ok-transfers-apply?": apply_ok})
            _, got = emu_check(emu, h, o2, seed, grid=2)
            assert_same(got, L.realtime_numpy(h, o2), (plant, apply_ok))


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h, o, _ = G.concurrent_ledger(1, ops=20, fail=0.0)
    accounts, init, apply_ok = L._rt_opts(None, o)
    cols = L.LedgerColumns(h)
    s, keep = L.ledger_rt_in(cols, accounts, init, apply_ok)
    s.ok_transfers_apply = 3
    out = N.LedgerRtOut()
    assert emu.emu_rt_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0)) == N.ERR_INVALID_ARG
    assert "ok_transfers_apply is 0 or 1" in emu.emu_rt_error().decode()
    t = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))[0]
    cols.mop_c[int(cols.mop_off[t])] = 2 ** 31
    s, keep = L.ledger_rt_in(cols, accounts, init, apply_ok)
    assert emu.emu_rt_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0)) == N.ERR_UNSUPPORTED and out.summary.bad_amounts == 1

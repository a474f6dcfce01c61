"""tbc_ledger_snapshots on the CPU: the host plan (csrc/ledger_snap_plan.h) and the kernels of csrc/ledger_snap_kernels.h -- the file
hipcc compiles into libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_ledger_snap.cpp lays the arena
out and runs the kernels in the library's launch order, every grid capped at 3 workgroups so that the grid strides run), against
snapshots_numpy of jepsen/ledger.py: every output array and every summary field, n_candidates included, exactly, under two seeded
interleavings of the wavefronts, on the shape cases of tests/test_ledger_snapshots_gpu.py (those of more than 16,000 reads are the
device's: here the plan's knobs reach the same paths -- one or two chunks for the sort, so that a chunk is several wavefronts' worth;
one sorted read per chunk of the scan, so that its carry takes a second step of 256 chunks).  Test infrastructure only: the product
has no CPU path."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import ledger_realtime_histories as G
import ledger_snapshot_histories as S
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

SEEDS = (1, 2)
CASES = S.shape_cases(big=False)
ARRAYS = ("count", "first", "key", "flags")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_snap") / "libemu_snap.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_ledger_snap.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_snap_check.restype = C.c_int
    lib.emu_snap_error.restype = C.c_char_p
    lib.emu_snap_pair_launches.restype = C.c_uint64
    return lib


def emu_check(lib, history, opts, seed, grid=3, sort_chunks_cap=0, scan_rows=0):
    accounts = L._snap_accounts(None, opts)
    cols = L.LedgerColumns(history)

    def call(s, out):
        st = lib.emu_snap_check(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed), C.c_uint32(sort_chunks_cap), C.c_uint32(scan_rows))
        assert st == 0, lib.emu_snap_error().decode()

    return cols, L.check_snapshots_native(cols, accounts, call=call)


def assert_same(got, want, tag):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")} == want["summary"], tag


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_numpy_statement(emu, case):
    h, o = case["history"], case["opts"]
    want = L.snapshots_numpy(h, o)
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert (want["summary"]["skewed"]["count"] if k == "skewed" else want["summary"][k]) == v, (case["name"], k)
    for seed in SEEDS:
        cols, got = emu_check(emu, h, o, seed)
        assert_same(got, want, (case["name"], seed))
        assert emu.emu_snap_pair_launches() == (1 if want["summary"]["n_candidates"] else 0)     # no candidate: no pair kernel
    # only the reads' micro-ops are copied, 25 bytes each
    rd = (cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ)
    n_read_mops = int((cols.mop_off[1:][rd] - cols.mop_off[:-1][rd]).sum())
    assert 25 * n_read_mops <= got["summary"]["bytes_in"] <= 25 * n_read_mops + 8 * len(cols.read_ops) + 12 * len(o["accounts"]) + 16 * 256
    assert L.snapshots_result_map(h, cols, got, o["accounts"]) == L._snap_map(h, cols.read_ops, want, o["accounts"])


def test_the_plan_cuts_where_the_cases_say(emu):
    for n, sort_chunks, scan_chunks in ((63, 1, 1), (64, 1, 1), (65, 2, 2), (129, 3, 3), (257, 5, 5)):
        name = f"chain-of-{n}" if n < 200 else f"antichain-of-{n}"
        h, o = next((c["history"], c["opts"]) for c in CASES if c["name"] == name)
        s, keep = L.ledger_snap_in(L.LedgerColumns(h), o["accounts"])
        shape = (C.c_uint64 * 8)()
        assert emu.emu_snap_shape(C.byref(s), shape) == 0
        assert [int(x) for x in shape[:7]] == [n, 2 * len(o["accounts"]), n * len(o["accounts"]), sort_chunks, 64, 64, scan_chunks]


@pytest.mark.parametrize("name", ["chain-of-129", "antichain-of-300", "one-outlier", "partial-reads-only", "complete-skewed-with-partial-only",
                                  "sums-every-byte", "sums-highest-byte-and-sign", "planted-fork", "planted-torn", "identical-reads"])
def test_chunks_of_several_wavefronts_and_a_carry_of_several_steps(emu, name):
    """what the device meets past 16,384 reads: a chunk of the sort that takes several steps of 64 reads (the digit's base moves from step
    to step in LDS), and more than 256 chunks of the scan (the carried maximum and minimum go from one step of 256 chunks to the next)"""
    case = next(c for c in CASES if c["name"] == name)
    want = L.snapshots_numpy(case["history"], case["opts"])
    assert want["summary"]["read_count"] > 64
    for seed, cap in zip(SEEDS, (1, 2)):
        _, got = emu_check(emu, case["history"], case["opts"], seed, grid=2, sort_chunks_cap=cap, scan_rows=1 if want["summary"]["read_count"] > 256 else 3)
        assert_same(got, want, (name, seed, cap))


def test_random_vectors_with_partial_reads(emu):
    rng = random.Random(17)
    for trial in range(12):
        accounts = rng.sample(range(1, 60), rng.choice((1, 2, 5, 17)))
        h, o = S.reads_ledger(accounts, S.random_rows(rng, accounts, rng.randint(1, 150)), transfers_first=trial % 3)
        _, got = emu_check(emu, h, o, trial, grid=2, scan_rows=(0, 5)[trial % 2])
        assert_same(got, L.snapshots_numpy(h, o), trial)


def test_random_concurrent_ledgers_are_valid_and_launch_no_pair_kernel(emu):
    for seed, plant in enumerate([(), ("stale",), ("future", "regressed"), G.ANOMALIES]):
        h, o, planted = G.concurrent_ledger(40 + seed, workers=6, ops=120, plant=plant)
        _, got = emu_check(emu, h, o, seed, grid=2)
        assert_same(got, L.snapshots_numpy(h, o), plant)
        assert got["summary"]["valid"] == 1 and got["summary"]["n_candidates"] == 0 and emu.emu_snap_pair_launches() == 0
        assert got["summary"]["n_checked"] == 8 * got["summary"]["read_count"] > 0


def test_no_accounts_at_all(emu):
    """what only a direct caller of the C entry can ask: no account, so no counter: every read is complete and nothing is skewed"""
    h, o, _ = G.concurrent_ledger(5, ops=40)
    cols = L.LedgerColumns(h)

    def call(s, out):
        assert emu.emu_snap_check(C.byref(s), C.byref(out), C.c_uint32(2), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0)) == 0, emu.emu_snap_error().decode()

    got = L.check_snapshots_native(cols, [], call=call)
    want = L.snapshots_dense_numpy(*L._snap_dense(cols, []))
    assert_same(got, want, "no accounts")
    assert got["summary"]["n_checked"] == 0 and got["summary"]["n_partial"] == 0 and got["summary"]["read_count"] == len(cols.read_ops) > 0


def test_magnitudes_that_reach_2_to_the_63_are_counted_on_the_device(emu):
    h, o = S.reads_ledger([1, 2], S.chain_rows([1, 2], 70))
    for values, bad in (((2 ** 62, 2 ** 62), 1), ((-(2 ** 63), 0), 1), ((2 ** 62, 2 ** 62 - 3), 0)):
        cols = L.LedgerColumns(h)
        m = int(cols.mop_off[np.flatnonzero((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ))[66]])
        cols.mop_a[m], cols.mop_b[m] = values
        cols.mop_a[m + 1], cols.mop_b[m + 1] = 1, 1
        s, keep = L.ledger_snap_in(cols, o["accounts"])
        out = N.LedgerSnapOut()
        flags = np.full(70, 77, np.uint8)
        out.snap_flags = flags.ctypes.data_as(C.POINTER(C.c_uint8))
        st = emu.emu_snap_check(C.byref(s), C.byref(out), C.c_uint32(2), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0))
        assert (st, out.summary.bad_values) == ((N.ERR_UNSUPPORTED, 1) if bad else (0, 0)), values
        assert (flags == 77).all() == bool(bad)                               # no results


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h, o, _ = G.concurrent_ledger(1, ops=20)
    cols = L.LedgerColumns(h)
    s, keep = L.ledger_snap_in(cols, o["accounts"])
    keep["type"][3] = 9
    out = N.LedgerSnapOut()
    assert emu.emu_snap_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0)) == N.ERR_INVALID_ARG
    assert "op 3 (index" in emu.emu_snap_error().decode()

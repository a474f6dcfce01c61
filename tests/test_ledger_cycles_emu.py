"""tbc_ledger_cycles on the CPU: the host plan (csrc/ledger_cycles_plan.h) and the kernels of csrc/ledger_cycles_kernels.h -- the file
hipcc compiles into libtbcheck.so, the snapshot filter's kernels with it -- under the wavefront / workgroup emulator of tests/emu
(tests/emu/emu_ledger_cycles.cpp lays the arena out and runs the kernels in the library's launch order, every grid capped at 3
workgroups so that the grid strides run), against cycles_numpy of jepsen/ledger.py: both output arrays and every summary field,
closure_rounds included, exactly, under two seeded interleavings of the wavefronts, on the curated histories of
tests/ledger_cycle_histories.py and on random ones; with the plan's knobs, sort chunks of several wavefronts' worth and scan carries of
several steps.  Test infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import random
import subprocess

import pytest

import ledger_cycle_histories as CH
import ledger_realtime_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L
from test_ledger_cycles_host import assert_same

SEEDS = (1, 2)
CASES = CH.cases()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_cycles") / "libemu_cycles.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_ledger_cycles.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_cycles_check.restype = C.c_int
    lib.emu_cycles_error.restype = C.c_char_p
    lib.emu_cycles_launches.restype = C.c_uint64
    return lib


def emu_check(lib, history, opts, seed, grid=3, sort_chunks_cap=0, scan_rows=0, max_core=0):
    cols = L.LedgerColumns(history)

    def call(s, out):
        st = lib.emu_cycles_check(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed), C.c_uint32(sort_chunks_cap), C.c_uint32(scan_rows), C.c_uint32(max_core))
        assert st in (0, N.ERR_UNSUPPORTED), lib.emu_cycles_error().decode()
        return st

    return cols, L.check_cycles_native(cols, L._snap_accounts(None, opts), call=call)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_numpy_statement(emu, case):
    h, o = case["history"], case["opts"]
    want = L.cycles_numpy(h, o)
    for seed in SEEDS:
        cols, got = emu_check(emu, h, o, seed)
        assert_same(got, want, (case["name"], seed))
        m = want["summary"]["n_core"]
        # no core: no matrix, no closure, no member kernel; otherwise one matrix kernel and a closure kernel a round
        assert [emu.emu_cycles_launches(k) for k in range(3)] == [want["summary"]["closure_rounds"], int(m > 0), int(m > 0)]
    assert L.cycles_result_map(h, cols, got, o["accounts"]) == L._cyc_map(h, want, o["accounts"])


@pytest.mark.parametrize("name", ["65-reads-cycle-of-5", "core-cycle-of-65", "core-path-of-70-closed", "core-path-of-70-open", "all-complete-valid",
                                  "all-complete-long-fork", "all-complete-regressed"])
def test_chunks_of_several_wavefronts_and_a_carry_of_several_steps(emu, name):
    case = next(c for c in CASES if c["name"] == name)
    want = L.cycles_numpy(case["history"], case["opts"])
    assert want["summary"]["read_count"] > 50
    for seed, cap in zip(SEEDS, (1, 2)):
        _, got = emu_check(emu, case["history"], case["opts"], seed, grid=2, sort_chunks_cap=cap, scan_rows=3)
        assert_same(got, want, (name, seed, cap))


def test_random_histories(emu):
    rng = random.Random(23)
    for trial in range(120):
        h, o = CH.random_history(rng)
        _, got = emu_check(emu, h, o, trial, grid=1 + trial % 3, scan_rows=(0, 2)[trial % 2])
        assert_same(got, L.cycles_numpy(h, o), (trial, h, o))


def test_more_reads_than_a_step_of_the_scans(emu):
    """more than 256 reads: the one-workgroup scans carry from step to step; a core of more than 256: the matrix's rows take several
    steps of columns, the component kernel several steps of members"""
    rng = random.Random(4)
    accounts, rows = CH.core_path(300, True, 2)
    extra = [CH.full(accounts, 9 + k // 2) for k in range(30)]
    rows = rows[:150] + extra + rows[150:]
    h, o = CH.concurrent(accounts, rows)
    want = L.cycles_numpy(h, o)
    assert want["summary"]["n_core"] == 300 and want["summary"]["n_on_cycle"] == 300 and want["summary"]["read_count"] == 332
    _, got = emu_check(emu, h, o, 1, grid=2)
    assert_same(got, want, "300")
    rows = [CH.full([1, 2], k // 3) for k in range(600)]
    for k in rng.sample(range(600), 25):
        rows[k] = [(1, rng.randrange(200), rng.randrange(200))]
    h, o = CH.timed_reads([1, 2], [(row, 2 * k, 2 * k + 1) for k, row in enumerate(rows)])       # one after the other
    want = L.cycles_numpy(h, o)
    assert want["summary"]["n_partial"] == 25 and want["summary"]["n_on_cycle"] > 25
    _, got = emu_check(emu, h, o, 2, grid=3, sort_chunks_cap=2)
    assert_same(got, want, "600")


def test_valid_concurrent_ledgers_have_no_core_and_launch_no_closure(emu):
    for seed in range(3):
        h, o, _ = G.concurrent_ledger(40 + seed, workers=6, ops=120)
        _, got = emu_check(emu, h, o, seed, grid=2)
        assert_same(got, L.cycles_numpy(h, o), seed)
        assert got["summary"]["valid"] == 1 and got["summary"]["n_core"] == 0 and got["summary"]["closure_rounds"] == 0
        assert [emu.emu_cycles_launches(k) for k in range(3)] == [0, 0, 0]


def test_a_core_above_the_cap_is_refused_with_its_size(emu):
    case = next(c for c in CASES if c["name"] == "core-cycle-of-33")
    cols, got = emu_check(emu, case["history"], case["opts"], 1, max_core=32)
    assert got["unsupported"] and got["summary"]["n_core"] == 33 and got["summary"]["read_count"] == 36 and got["summary"]["n_partial"] == 33
    assert L.cycles_result_map(case["history"], cols, got, case["opts"]["accounts"]) == {"valid?": "unknown", "searched?": False, "n-core": 33}
    _, got = emu_check(emu, case["history"], case["opts"], 1, max_core=33)
    assert not got.get("unsupported") and got["summary"]["n_on_cycle"] == 33


def test_magnitudes_that_reach_2_to_the_63_are_counted_on_the_device(emu):
    h, o = CH.concurrent([1, 2], [[(1, 2 ** 62, 2 ** 62), (2, 0, 0)], [(1, 1, 1)]])
    with pytest.raises(ValueError):
        emu_check(emu, h, o, 1)


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h, o, _ = G.concurrent_ledger(1, ops=20)
    cols = L.LedgerColumns(h)
    s, keep = L.ledger_rt_in(cols, o["accounts"], {a: (0, 0) for a in o["accounts"]})
    keep["type"][3] = 9
    out = N.LedgerCyclesOut()
    assert emu.emu_cycles_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)) == N.ERR_INVALID_ARG
    assert "op 3 (index" in emu.emu_cycles_error().decode()

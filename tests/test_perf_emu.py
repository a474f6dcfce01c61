"""tbc_perf_series on the CPU: the host plan (csrc/perf_plan.h) and the kernels of csrc/perf_kernels.h -- the file hipcc compiles into
libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_perf.cpp lays the arena out and runs the kernels
in the library's launch order, the select's LDS tile 32 latencies, every grid capped at 3 workgroups so that the grid strides run),
against the host statement of jepsen/perf.py: every output array and every summary field, exactly, under two seeded interleavings of
the wavefronts, on the shape cases of tests/perf_histories.py.  Test infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import subprocess

import pytest

import perf_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd.jepsen import perf as PF

SEEDS = (1, 2)
CASES = G.shape_cases()
TILE = 32


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_pf") / "libemu_pf.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_perf.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_pf_series.restype = lib.emu_pf_plan_sizes.restype = lib.emu_pf_shape.restype = C.c_int
    lib.emu_pf_error.restype = C.c_char_p
    lib.emu_pf_tile.restype = C.c_uint32
    assert lib.emu_pf_tile() == TILE
    return lib


@pytest.fixture(scope="module")
def refs():
    return G.references(CASES)


def emu_series(lib, history, seed, grid=3):
    cols = PF.PerfColumns(history)

    def call(s, out):
        assert lib.emu_pf_series(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed)) == 0, lib.emu_pf_error().decode()

    def sizes_call(s, z):
        assert lib.emu_pf_plan_sizes(C.byref(s), C.byref(z)) == 0, lib.emu_pf_error().decode()

    return cols, PF.check_native(cols, call=call, sizes_call=sizes_call)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_host_statement(emu, refs, case):
    h, want = case["history"], refs[case["name"]]
    for seed in SEEDS:
        cols, got = emu_series(emu, h, seed)
        G.assert_same(got, want, (case["name"], seed))
    # ... and the series named from those arrays are the host statement's own
    assert PF.series_from_device(h, cols, got) == PF.series_host(h), case["name"]


def test_the_cases_take_both_selects_and_several_chunks(emu, refs):
    """with the emulator's tile a cell of 33 and more takes the radix select, one of 32 and fewer the LDS sort; the open scan's cases span
    more chunks than the 3 workgroups the grid is capped at"""
    sizes = {int(x) for c in CASES for x in refs[c["name"]]["q_count"].reshape(-1)}
    assert {1, 2, 3, 20, 31, 32, 33, 34, 64, 65, 100, 101, 130} <= sizes
    for name in ("open_one_class_over_chunks", "open_two_classes_interleaved", "open_back_to_0_on_the_edge"):
        h = next(c["history"] for c in CASES if c["name"] == name)
        s, keep = PF.perf_in(PF.PerfColumns(h))
        shape = (C.c_uint64 * 6)()
        assert emu.emu_pf_shape(C.byref(s), shape) == 0
        assert shape[0] == 64 and shape[1] > 3, (name, list(shape))


def test_random_histories(emu):
    for seed in range(4):
        h = G.random_history(100 + seed, 700, workers=3 + 4 * seed, fs=("read", "write", "cas")[:1 + seed % 3], gap=(2_000_000, 40_000_000)[seed % 2],
                             info=0.1, jitter=(0, 3 * G.S)[seed // 2])
        _, got = emu_series(emu, h, seed, grid=2)
        G.assert_same(got, G.expected(h), seed)


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h = G.random_history(1, 20)
    cols = PF.PerfColumns(h)
    cols.time[7] = -5
    s, keep = PF.perf_in(cols)
    out = PF.N.PerfOut()
    assert emu.emu_pf_series(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1)) == PF.N.ERR_BAD_HISTORY
    assert "op 7: negative :time" in emu.emu_pf_error().decode()

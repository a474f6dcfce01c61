"""tbc_ledger_check on the CPU: the host plan (csrc/ledger_plan.h) and the kernels of csrc/ledger_kernels.h -- the file hipcc compiles
into libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_ledger.cpp lays the arena out and runs the
kernels in the library's launch order, the lookup window 8 words = 256 transfers, every grid capped at 3 workgroups so that the grid
strides run), against the host statement of jepsen/ledger.py: every output array and every summary field, exactly, under two seeded
interleavings of the wavefronts, on the shapes of tests/test_ledger_gpu.py (|T| of 0, 1, 255..257 = 32 x 8 +- 1 among them).  Test
infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import subprocess

import pytest

import ledger_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd.jepsen import ledger as L

SEEDS = (1, 2)
CASES = G.shape_cases()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_lg") / "libemu_lg.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_ledger.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_lg_check.restype = C.c_int
    lib.emu_lg_error.restype = C.c_char_p
    lib.emu_lg_window_words.restype = C.c_uint32
    assert lib.emu_lg_window_words() == 8
    return lib


@pytest.fixture(scope="module")
def refs():
    return G.references(CASES)


def emu_check(lib, history, opts, seed, grid=3):
    accounts, total, neg = L._si_opts(None, opts)
    cols = L.LedgerColumns(history, total)

    def call(s, out):
        assert lib.emu_lg_check(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed)) == 0, lib.emu_lg_error().decode()

    return cols, L.check_native(cols, accounts, neg, call=call)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_host_statement(emu, refs, case):
    name = case["name"]
    if "runs" in case:                                                        # the plan cuts the reads into the runs the case is named for
        cols = L.LedgerColumns(case["history"], case["opts"]["total-amount"])
        s, keep = L.ledger_in(cols, case["opts"]["accounts"])
        shape = (C.c_uint64 * 6)()
        assert emu.emu_lg_shape(C.byref(s), shape) == 0
        assert (len(cols.read_ops), int(shape[0]), int(shape[1])) == (case["ok_reads"], case["ok_reads"], case["runs"])
    for neg in (False, True):
        h, o, want = refs[(name, neg)]
        for seed in SEEDS:
            cols, got = emu_check(emu, h, o, seed)
            G.assert_same(got, want, (name, neg, seed))
        # ... and the result maps made from those arrays are the host checkers' own
        maps = L.result_maps(h, cols, got, o["accounts"], neg)
        assert maps == {"SI": L.BankChecker(o).check(o, h), "lookup-transfers": L.LookupAllInvokedTransfers().check(o, h),
                        "final-reads": L.FinalReads().check(o, h)}, name


def test_random_ledgers_with_every_planted_anomaly(emu):
    plants = [(), ("wrong-total", "negative"), ("unexpected", "nil", "dup-id"), ("missing-transfer",), ("final-read-field", "final-lookup-order"),
              ("final-read-order", "final-lookup-field"), ("final-lookup-length", "final-read-length"), ("no-final",),
              ("wrong-total", "negative", "unexpected", "nil", "dup-id", "final-read-length", "final-lookup-field")]
    inputs = [G.random_ledger(seed, workers=5, transfers=60, reads=80, info=0.04 * (seed % 2), fail=0.03 * (seed % 2), plant=p)
              for seed, p in enumerate(plants)]
    wants = [G.expected(h, o) for h, o in inputs]
    for (h, o), want, p in zip(inputs, wants, plants):                        # every plant has landed, and the plain input is fully valid
        assert set(p or ("valid",)) <= G.landed(h, want["summary"]), (p, G.landed(h, want["summary"]))
    assert set().union(*plants) == set(G.ANOMALIES)
    for seed, ((h, o), want) in enumerate(zip(inputs, wants)):
        _, got = emu_check(emu, h, o, seed, grid=2)
        G.assert_same(got, want, plants[seed])


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h, o = G.random_ledger(1, transfers=5, reads=4)
    cols = L.LedgerColumns(h, o["total-amount"])
    s, keep = L.ledger_in(cols, [1, 2, 2])
    out = L.N.LedgerOut()
    assert emu.emu_lg_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1)) == 1
    assert "account 2 is listed twice" in emu.emu_lg_error().decode()

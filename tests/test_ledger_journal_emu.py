"""tbc_ledger_journal on the CPU: the host plan (csrc/ledger_journal_plan.h) and the kernels of csrc/ledger_journal_kernels.h -- the file
hipcc compiles into libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_ledger_journal.cpp lays the
arena out and runs the kernels in the library's launch order, every grid capped at 3 workgroups so that the grid strides run), against
journal_numpy of jepsen/ledger.py: every output array and every summary field, exactly, under two seeded interleavings of the
wavefronts, on the shape cases of tests/ledger_journal_histories.py.  The cases sized by the library's constants are the device's: here
the plan's knobs reach the same paths -- 7 entries a slice, so that a lookup is sliced over several workgroups whose rows are OR-ed; 64
micro-ops a chunk of the members kernel; an LDS window of 3 words, so that every record past the 96th takes the global path.  Test
infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import ledger_journal_histories as J
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

SEEDS = (1, 2)
assert_same, bytes_bound = J.assert_same, J.bytes_bound
CASES = J.shape_cases(big=False)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_journal") / "libemu_journal.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_ledger_journal.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_journal_check.restype = C.c_int
    lib.emu_journal_error.restype = C.c_char_p
    return lib


def emu_check(lib, history, opts, seed, grid=3, slice_entries=7, chunk=64):
    accounts, init, apply_ok = L._rt_opts(None, opts)
    cols = L.LedgerColumns(history)

    def call(s, out):
        st = lib.emu_journal_check(C.byref(s), C.byref(out), C.c_uint32(grid), C.c_uint64(seed), C.c_uint32(slice_entries), C.c_uint32(chunk))
        assert st == 0, lib.emu_journal_error().decode()

    return cols, L.check_journal_native(cols, accounts, init, apply_ok, call=call)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_emulator_equals_numpy_statement(emu, case):
    h, o = case["history"], case["opts"]
    want = L.journal_numpy(h, o)
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        have = want["summary"]["totals"][k] if k in L.JN_KINDS else want["summary"][k]
        assert have > 0 if v == ">0" else have == v, (case["name"], k, have)
    for seed in SEEDS:
        cols, got = emu_check(emu, h, o, seed)
        assert_same(got, want, (case["name"], seed))
    lo, hi = bytes_bound(cols, len(o["accounts"]))
    assert lo <= got["summary"]["bytes_in"] <= hi
    assert L.journal_result_map(h, cols, got) == L._jn_map(h, want)


def test_the_plan_cuts_where_the_knobs_say(emu):
    case = next(c for c in CASES if c["name"] == "65-entries")
    accounts, init, apply_ok = L._rt_opts(None, case["opts"])
    s, keep = L.ledger_rt_in(L.LedgerColumns(case["history"]), accounts, init, apply_ok)
    shape = (C.c_uint64 * 11)()
    for (slice_entries, chunk), (slices, chunk_is) in {(0, 0): (1, 256), (7, 64): (10, 64), (64, 100): (2, 64), (65, 1000): (1, 256)}.items():
        assert emu.emu_journal_shape(C.byref(s), C.c_uint32(slice_entries), C.c_uint32(chunk), shape) == 0
        assert [int(x) for x in shape[:9]] == [65, 3, 65, 1, slices, slice_entries or 4096, chunk_is, 2, 16]


@pytest.mark.parametrize("knobs", [(1, 1, 64), (2, 3, 128), (3, 0, 0)], ids=str)
def test_slices_chunks_and_grids_of_other_sizes(emu, knobs):
    grid, slice_entries, chunk = knobs
    for name in ("65-lookups", "257-entries", "ok-fail-info-open", "planted-ahead-of-journal", "1025-accounts"):
        case = next(c for c in CASES if c["name"] == name)
        _, got = emu_check(emu, case["history"], case["opts"], 5, grid=grid, slice_entries=slice_entries, chunk=chunk)
        assert_same(got, L.journal_numpy(case["history"], case["opts"]), (name, knobs))


def test_random_concurrent_ledgers_plain_and_planted(emu):
    for seed in range(4):
        h, o, meta = J.journal_ledger(50 + seed, workers=3 + seed, ops=90, fail=0.1 * (seed % 2))
        _, got = emu_check(emu, h, o, seed, grid=2)
        assert_same(got, L.journal_numpy(h, o), seed)
        s = got["summary"]
        assert s["n_checked"] == 8 * s["read_count"] > 0 and s["n_entries"] > 0 and got["lk_present"].sum() > 0
        assert s["valid"] == 1 or seed % 2                                     # (a failed transfer is in no lookup: nothing the audit reports)
    rng = random.Random(3)
    for trial in range(6):                                                     # random damage: entries dropped, doubled, changed, made up
        h, o, meta = J.journal_ledger(60 + trial, workers=4, ops=70)
        for Lk in meta["lookups"]:
            v = h[Lk["ret"]]["value"] = [list(m[:2]) + [dict(m[2])] for m in h[Lk["ret"]]["value"]]
            for _ in range(rng.randint(0, 3)):
                k = rng.randrange(len(v))
                how = rng.randrange(5)
                if how == 0 and len(v) > 1: del v[k]
                elif how == 1: v.append(v[k])
                elif how == 2: v[k][2]["amount"] += 1
                elif how == 3: v.append(["l-t", 10 ** 6 + k, dict(v[k][2])])
                else: v[k][2] = None
        _, got = emu_check(emu, h, o, trial, grid=2, slice_entries=5)
        assert_same(got, L.journal_numpy(h, o), ("damage", trial))


def test_amounts_out_of_range_are_counted_on_the_device(emu):
    case = next(c for c in CASES if c["name"] == "65-entries")
    accounts, init, apply_ok = L._rt_opts(None, case["opts"])
    for amount, bad in ((2 ** 31, 1), (-1, 1), (2 ** 31 - 1, 0)):
        cols = L.LedgerColumns(case["history"])
        tr = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))
        cols.mop_c[int(cols.mop_off[tr[40]])] = amount
        s, keep = L.ledger_rt_in(cols, accounts, init, apply_ok)
        out, arr, _ = L.journal_out(cols, len(accounts))
        for x in arr.values():
            x[:] = 77
        st = emu.emu_journal_check(C.byref(s), C.byref(out), C.c_uint32(2), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0))
        assert (st, out.summary.bad_amounts) == ((N.ERR_UNSUPPORTED, 1) if bad else (0, 0)), amount
        assert all((x == 77).all() for x in arr.values()) == bool(bad)          # no results


def test_the_emulator_refuses_what_the_library_refuses(emu):
    h, o, _ = J.journal_ledger(1, ops=30)
    accounts, init, apply_ok = L._rt_opts(None, o)
    s, keep = L.ledger_rt_in(L.LedgerColumns(h), accounts, init, apply_ok)
    keep["type"][3] = 9
    out = N.LedgerJournalOut()
    assert emu.emu_journal_check(C.byref(s), C.byref(out), C.c_uint32(1), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0)) == N.ERR_INVALID_ARG
    assert "op 3 (index" in emu.emu_journal_error().decode()

"""tbc_pair_events_batch on the CPU: the host plan and the step list of csrc/pair_plan.h and the kernels of csrc/pair_kernels.h -- the
file hipcc compiles into libtbcheck.so -- under the wavefront / workgroup emulator of tests/emu (tests/emu/emu_pair.cpp), against
tbc_pair_events history by history: every output array bit for bit on the shapes of tests/pair_events_shapes.py, with the grids capped
at 3 and at 1 workgroups (so that a workgroup's LDS tables serve one history after another).  A history belongs to ONE wavefront from
its first event to its last (pair_kernels.h, "the split"), so there is no interleaving of wavefronts within a history to vary; the
emulator's own check that every cross-lane primitive is met by all 64 lanes runs throughout.  Two planted mutations of the kernels
(PR_MUTATION) must each be seen by a shape.  The same program with its own main (EMU_PAIR_MAIN, linked with csrc/tbc_host.cpp) is
built and run here as a plain executable; built with -fsanitize=address,undefined in addition it runs the same way, outside Python.
Test infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pair_events_shapes as S
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N, columns

FLAGS = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "emu", "emu_pair.cpp")
CASES = sorted(S.cases())


@pytest.fixture(scope="module")
def emus(tmp_path_factory, native):
    d = tmp_path_factory.mktemp("emu_pr")
    procs, libs = [], {}
    for m in (0, 1, 2):
        so = str(d / f"libemu_pr{m}.so")
        procs.append((m, so, subprocess.Popen(FLAGS + ["-shared", "-fPIC"] + ([f"-DPR_MUTATION={m}"] if m else []) + [SRC, "-o", so])))
    for m, so, p in procs:
        assert p.wait() == 0
        lib = C.CDLL(so)
        lib.emu_pr_batch.restype = C.c_int
        lib.emu_pr_error.restype = C.c_char_p
        lib.emu_pr_hash.restype = lib.emu_pr_mutation.restype = C.c_uint32
        assert lib.emu_pr_mutation() == m
        libs[m] = lib
    return libs


def run(lib, evs, word=False, ops_cap=None, grid=3, seed=1, columns_wanted=True):
    ev_off, ev = columns.concat_events(evs)
    call = lambda i, o: lib.emu_pr_batch(i, o, C.c_uint32(grid), C.c_uint64(seed))
    st, got = columns.pair_events_batch_raw(ev_off, ev, ops_cap=ops_cap, word=word, columns=columns_wanted, call=call)
    return st, got, lib.emu_pr_error().decode()


@pytest.mark.parametrize("name", CASES)
def test_emulator_equals_tbc_pair_events(emus, name):
    evs = S.cases()[name]
    for word in ((False, True) if name in S.WORD_CASES else (False,)):
        want = S.reference(name, evs, word)
        for grid, seed in ((3, 1), (1, 2)):
            st, got, err = run(emus[0], evs, word=word, grid=grid, seed=seed)
            assert st == 0, err
            S.assert_same(got, want, (name, word, grid))


def test_the_shapes_hold_what_they_are_there_for(emus):
    c = S.cases()
    for k in (0, 1, 4096, 4097, 1 << 24, -1, -2 ** 31, 0x7FFFFFFF, 123456789):
        assert emus[0].emu_pr_hash(C.c_uint32(k & 0xFFFFFFFF)) == S.table_hash(k), k
    assert len({S.table_hash(k) for k in (1, 4096, 1 << 24)}) == 1 and S.table_hash(4097) == S.table_hash(0) and 4097 % S.TABLE == 1
    assert [len(e) for e in c["lengths"]][:8] == [0, 1, 2, 63, 64, 65, 128, 129] and len(c["lengths"][8]) > 64 * 64
    edge = c["chunk_edges"][0]
    assert (edge.type[63], edge.process[63], edge.type[64], edge.process[64]) == (S.I, 7, S.OK, 7)
    ref = S.reference("processes_4096_and_4097", c["processes_4096_and_4097"], True)
    assert list(ref["status"]) == [0, N.ERR_UNSUPPORTED, 0, 0, N.ERR_UNSUPPORTED] and list(ref["n_process"]) == [4096, 0, 3, 4096, 0]
    ref = S.reference("malformed_each", c["malformed_each"], False)
    assert (ref["status"] == N.ERR_BAD_HISTORY).all() and list(ref["bad_row"]) == [91, 92, 90, 90, 0, 0, 92, 92] and ref["n_ops"] == 0
    ref = S.reference("malformed_two", c["malformed_two"], False)
    assert list(ref["bad_row"]) == [70, 71, 10, 63, 64, 129]
    ref = S.reference("bad_among_good", c["bad_among_good"], False)
    assert list(ref["status"] != 0) == [True, False, False, True, False, False, True]
    ref = S.reference("wire", c["wire"], True)
    assert list(ref["status"]) == [0, 0, N.ERR_UNSUPPORTED, N.ERR_UNSUPPORTED, N.ERR_UNSUPPORTED, 0, 0, N.ERR_UNSUPPORTED]
    ref = S.reference("refusal_precedence", c["refusal_precedence"], False)
    B, U = N.ERR_BAD_HISTORY, N.ERR_UNSUPPORTED
    assert list(ref["status"]) == [B, U, B, U, U, B] and list(ref["bad_row"]) == [0, N.PAIR_NO_ROW, 4096, N.PAIR_NO_ROW, N.PAIR_NO_ROW, 4096 + 64]
    ref = S.reference("semantics", c["semantics"], False)
    assert (ref["status"] == 0).all() and ref["n_process"][3] == 0 and ref["op_off"][4] == ref["op_off"][3]


def test_capacity_exact_and_one_below(emus):
    evs = S.cases()["bad_among_good"]
    want = S.reference("bad_among_good", evs, True)
    T = want["n_ops"]
    st, got, err = run(emus[0], evs, word=True, ops_cap=T)
    assert st == 0, err
    S.assert_same(got, want, "cap = need")
    ev_off, ev = columns.concat_events(evs)
    guard = {k: np.full(T + 7, 0xA5, dt) for k, dt in (("f", np.uint8), ("a", np.int32), ("inv_pos", np.uint32), ("ret_pos", np.uint32), ("word", np.uint32))}
    before = {k: v.copy() for k, v in guard.items()}
    i, o, keep = S.structs(ev_off, ev, T - 1, guard)
    assert emus[0].emu_pr_batch(C.byref(i), C.byref(o), C.c_uint32(3), C.c_uint64(1)) == N.ERR_INVALID_ARG
    assert f"{T} ops survive" in emus[0].emu_pr_error().decode()
    for k, v in guard.items():
        assert np.array_equal(v, before[k]), k


def test_only_the_arrays_asked_for(emus):
    evs = S.cases()["semantics"]
    want = S.reference("semantics", evs, False)
    st, got, err = run(emus[0], evs, columns_wanted=False)
    assert st == 0, err
    assert "f" not in got and "word" not in got
    S.assert_same(got, {k: v for k, v in want.items() if k not in ("f", "a", "b", "process")}, "descriptors and positions only")
    st, got, err = run(emus[0], [])
    assert st == 0 and got["n_ops"] == 0 and list(got["op_off"]) == [0], err


def test_random_histories_in_one_call(emus):
    evs = S.random_batch()
    want = S.reference("random", evs, True)
    assert (want["status"] == 0).all() and want["n_ops"] > 20000 and (want["ret_pos"] == N.POS_CRASHED).sum() > 100
    st, got, err = run(emus[0], evs, word=True, grid=5)
    assert st == 0, err
    S.assert_same(got, want, "random")


@pytest.mark.parametrize("mutation, seen_by", [(1, "chunk_edges"), (2, "semantics")])
def test_planted_mutations_are_seen(emus, mutation, seen_by):
    """1: a slot's carried state is not stored from lane 63 (an invocation there, its completion in the next chunk); 2: dense process
    numbers by first appearance among all invocations, not among the survivors"""
    evs = S.cases()[seen_by]
    st, got, err = run(emus[mutation], evs)
    assert st == 0, err
    with pytest.raises(AssertionError):
        S.assert_same(got, S.reference(seen_by, evs, False), seen_by)
    st, good, err = run(emus[0], evs)
    S.assert_same(good, S.reference(seen_by, evs, False), seen_by)


def test_stand_alone_program(tmp_path):
    """emu_pair.cpp with its own main and the specification linked in: a plain executable, built with the undefined-behaviour sanitizer
    (the same line with -fsanitize=address,undefined is the form for a machine where nothing else is preloaded into the process: the
    address sanitizer's runtime insists on being the first library loaded)"""
    exe = str(tmp_path / "emu_pair")
    subprocess.check_call(FLAGS + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DEMU_PAIR_MAIN", "-D__host__=", "-D__device__=", SRC, os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc", "tbc_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout + out.stderr

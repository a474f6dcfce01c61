"""The packed reader of csrc/pair_kernels.h on the CPU (tests/emu/emu_pair_packed.cpp): the kernels hipcc compiles into libtbcheck.so,
reading TBC_EVENT_WORD + process instead of the five columns, under the wavefront / workgroup emulator through the one-shot step list
of csrc/pair_plan.h, grids capped at 3 and at 1 -- bit for bit tbc_pair_events over what the words decode to (packed_events_shapes:
descriptors, status, bad row, wire word, positions).  A second entry lays the arena out as a batch does and emits into a separate stage
buffer: its thirds must equal the one-shot outputs, the words around them stay as they were, and a refused input writes nothing.  One
planted mutation (PR_MUTATION 3: the completion's type read from the invocation's word) must be seen by a shape.  The same program
with its own main is built with -fsanitize=address,undefined and run as a plain executable.  Test infrastructure only: the product has
no CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import packed_events_shapes as P
import pair_events_shapes as S
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N, columns

FLAGS = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "emu", "emu_pair_packed.cpp")
CASES = sorted(P.cases())
GUARD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def emus(tmp_path_factory, native):
    d = tmp_path_factory.mktemp("emu_prp")
    procs, libs = [], {}
    for m in (0, 3):
        so = str(d / f"libemu_prp{m}.so")
        procs.append((m, so, subprocess.Popen(FLAGS + ["-shared", "-fPIC"] + ([f"-DPR_MUTATION={m}"] if m else []) + [SRC, "-o", so])))
    for m, so, p in procs:
        assert p.wait() == 0
        lib = C.CDLL(so)
        lib.emu_prp_batch.restype = lib.emu_prp_stage.restype = C.c_int
        lib.emu_prp_error.restype = C.c_char_p
        lib.emu_prp_mutation.restype = C.c_uint32
        assert lib.emu_prp_mutation() == m
        libs[m] = lib
    return libs


def run(lib, evs, ops_cap=None, grid=3, seed=1):
    ev_off, words, process = P.concat_packed(evs)
    call = lambda i, o: lib.emu_prp_batch(i, o, C.c_uint32(grid), C.c_uint64(seed))
    st, got = columns.pair_events_batch_raw(ev_off, (words, process), ops_cap=ops_cap, word=True, call=call)
    return st, got, lib.emu_prp_error().decode()


def run_stage(lib, evs, ops_cap, spare=(2, 77), grid=3, seed=1):
    """-> (status, descriptors, the stage buffer of 3 * ops_cap words and 4 guard words behind it, the error text)"""
    ev_off, words, process = P.concat_packed(evs)
    nh = len(evs)
    i = N.PackedEventBatch()
    i.n_hist, i.device, i.ev_off = nh, 0, columns._p(ev_off, C.c_uint64)
    i.ev_word, i.process = columns._p(words, C.c_uint32), columns._p(process, C.c_int32)
    d = {"op_off": np.zeros(nh + 1, np.uint64), "n_events": np.zeros(nh, np.uint32), "n_process": np.zeros(nh, np.uint32),
         "status": np.zeros(nh, np.int32), "bad_row": np.zeros(nh, np.uint32)}
    o = N.PairOut()
    for k, ct in (("op_off", C.c_uint64), ("n_events", C.c_uint32), ("n_process", C.c_uint32), ("status", C.c_int32), ("bad_row", C.c_uint32)):
        setattr(o, k, columns._p(d[k], ct))
    stage = np.full(3 * ops_cap + 4, GUARD, np.uint32)
    st = lib.emu_prp_stage(C.byref(i), C.c_uint32(nh + spare[0]), C.c_uint64(len(words) + spare[1]), C.c_uint64(ops_cap), columns._p(stage, C.c_uint32),
                           C.byref(o), C.c_uint32(grid), C.c_uint64(seed))
    d.update(n_bad=int(o.n_bad), n_ops=int(o.n_ops))
    return st, d, stage, lib.emu_prp_error().decode()


@pytest.mark.parametrize("name", CASES)
def test_packed_reader_equals_tbc_pair_events(emus, name):
    evs = P.cases()[name]
    want = P.packed_reference(name, evs)
    for grid, seed in ((3, 1), (1, 2)):
        st, got, err = run(emus[0], evs, grid=grid, seed=seed)
        assert st == 0, err
        S.assert_same(got, want, (name, grid))


def test_the_new_shapes_hold_what_they_are_there_for(emus):
    c = P.cases()
    ref = P.packed_reference("packed_type_codes", c["packed_type_codes"])
    B = N.ERR_BAD_HISTORY
    assert list(ref["status"]) == [0, B, 0, B, 0, B, B] and list(ref["bad_row"][[1, 3, 5, 6]]) == [12, 70, 5, 5]
    evs = c["packed_field_edges"]
    ref = P.packed_reference("packed_field_edges", evs)
    st = {}
    for h, e in enumerate(evs):
        if len(e) == 19 and e.process[10] == 9:
            st[(int(e.type[11]), int(e.f[10]), int(e.a[10]), int(e.b[10]))] = int(ref["status"][h])
    U = N.ERR_UNSUPPORTED
    assert len(st) == 3 * 18
    for done in (S.OK, S.INFO):          # a surviving op, completed or crashed: what the wire format does not hold refuses the history
        assert [st[(done, f, 1, 0)] for f in (15, 16, 255)] == [0, U, U]
        assert [st[(done, S.W, a, 0)] for a in (254, 255, 256, -1, S.NIL)] == [0, U, U, U, 0]
        assert [st[(done, S.CAS, 1, b)] for b in (254, 255, 256, -1, S.NIL)] == [0, U, U, U, 0]
        assert [st[(done, S.W, 1, b)] for b in (254, 255, 256, -1, S.NIL)] == [0, 0, 0, 0, 0]
    assert all(v == 0 for k, v in st.items() if k[0] == S.FAIL)          # a failed op with such a value is still fine
    assert ref["n_ops"] > 0 and (ref["ret_pos"] == N.POS_CRASHED).sum() >= 10


def test_capacity_exact_and_one_below(emus):
    evs = P.cases()["bad_among_good"]
    want = P.packed_reference("bad_among_good", evs)
    T = want["n_ops"]
    st, got, err = run(emus[0], evs, ops_cap=T)
    assert st == 0, err
    S.assert_same(got, want, "cap = need")
    st, got, err = run(emus[0], evs, ops_cap=T - 1)
    assert st == N.ERR_INVALID_ARG and f"{T} ops survive" in err


def test_random_histories_in_one_call(emus):
    evs = S.random_batch()
    want = P.packed_reference("random", evs)
    assert (want["status"] == 0).all() and want["n_ops"] > 20000
    st, got, err = run(emus[0], evs, grid=5)
    assert st == 0, err
    S.assert_same(got, want, "random")
    assert got["bytes_in"] == 8 * sum(len(e) for e in evs) + 8 * (len(evs) + 1)


GOOD = ("lengths", "chunk_edges", "semantics", "jepsen_renumbering", "process_ids")


@pytest.mark.parametrize("name", GOOD)
def test_batch_layout_emits_the_one_shot_outputs_into_the_stage(emus, name):
    evs = [e for e in P.cases()[name] if len(e)]
    want = P.packed_reference(name + "/nonempty", evs)
    assert (want["status"] == 0).all()
    T = want["n_ops"]
    for cap, grid, seed in ((T, 3, 1), (T + 9, 1, 2)):
        st, d, stage, err = run_stage(emus[0], evs, cap, grid=grid, seed=seed)
        assert st == 0, err
        assert d["n_ops"] == T and d["n_bad"] == 0
        for k in ("op_off", "n_events", "n_process", "status", "bad_row"):
            assert np.array_equal(d[k], want[k]), (name, k)
        for third, k in enumerate(("word", "inv_pos", "ret_pos")):
            part = stage[third * cap:(third + 1) * cap]
            assert np.array_equal(part[:T], want[k]), (name, k, cap)
            assert (part[T:] == GUARD).all(), (name, k, "the words behind the ops")
        assert (stage[3 * cap:] == GUARD).all()


@pytest.mark.parametrize("name, status", [("bad_among_good", N.ERR_BAD_HISTORY), ("wire", N.ERR_UNSUPPORTED), ("packed_field_edges", N.ERR_UNSUPPORTED),
                                          ("packed_type_codes", N.ERR_BAD_HISTORY), ("refusal_precedence", N.ERR_BAD_HISTORY)])
def test_a_refused_input_writes_nothing_to_the_stage(emus, name, status):
    evs = P.cases()[name]
    want = P.packed_reference(name, evs)
    st, d, stage, err = run_stage(emus[0], evs, want["n_ops"] + 50)
    assert st == status, err
    assert (stage == GUARD).all()
    assert np.array_equal(d["status"], want["status"]) and np.array_equal(d["bad_row"], want["bad_row"]) and d["n_bad"] == want["n_bad"]
    first = int(np.flatnonzero(want["status"] == status)[0])
    assert f"history {first} " in err
    if status == N.ERR_BAD_HISTORY:
        assert f"row {int(want['bad_row'][first])}" in err


def test_more_ops_than_the_stage_holds_writes_nothing(emus):
    evs = P.cases()["semantics"]
    T = P.packed_reference("semantics", evs)["n_ops"]
    st, d, stage, err = run_stage(emus[0], evs, T - 1)
    assert st == N.ERR_INVALID_ARG and f"{T} ops survive" in err and (stage == GUARD).all()


def test_planted_mutation_is_seen(emus):
    """3: the completion's type read from the invocation's word -- no op fails, none completes"""
    evs = P.cases()["semantics"]
    want = P.packed_reference("semantics", evs)
    st, got, err = run(emus[3], evs)
    assert st == 0, err
    with pytest.raises(AssertionError):
        S.assert_same(got, want, "semantics")
    st, good, err = run(emus[0], evs)
    S.assert_same(good, want, "semantics")


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """(the sanitizers' runtimes are linked into the program itself, so nothing has to be loaded before it)"""
    exe = str(tmp_path / "emu_pair_packed")
    subprocess.check_call(FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-DEMU_PAIR_PACKED_MAIN",
                                   "-D__host__=", "-D__device__=", SRC, os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc", "tbc_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count("ok:") == 2 and "WRONG" not in out.stdout, out.stdout + out.stderr

"""tbc_pair_keyed_events on the CPU: the plan and the step list of csrc/split_plan.h and the kernels of csrc/split_kernels.h followed by
those of csrc/pair_kernels.h -- the files hipcc compiles into libtbcheck.so -- under the wavefront / workgroup emulator
(tests/emu/emu_split.cpp), against columns.split_events in numpy and tbc_pair_events key by key: every output array bit for bit on
the shapes of tests/keyed_events_shapes.py, with the grids capped at 3 and at 1 workgroups.  The program's own launcher runs the
workgroups of every launch in a seeded PERMUTED order, two seeds at least, so that a row's place taken from the order in which atomics
arrive would show on the CPU.  Four planted mutations of the kernels (SPLIT_MUTATION) must each be seen by a shape -- the third
only past 2^20 rows (keyed_events_shapes.large_cases, the split alone and once each), the fourth only where a probe run crosses
the table's end.  The same program
with its own main (EMU_SPLIT_MAIN, linked with csrc/tbc_host.cpp) is built with -fsanitize=address,undefined and run as a plain
executable, outside Python.  Test infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keyed_events_shapes as S
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N, columns

FLAGS = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "emu", "emu_split.cpp")
CASES = sorted(S.cases())


@pytest.fixture(scope="module")
def emus(tmp_path_factory, native):
    d = tmp_path_factory.mktemp("emu_sp")
    procs, libs = [], {}
    for m in (0, 1, 2, 3, 4):
        so = str(d / f"libemu_sp{m}.so")
        procs.append((m, so, subprocess.Popen(FLAGS + ["-shared", "-fPIC"] + ([f"-DSPLIT_MUTATION={m}"] if m else []) + [SRC, "-o", so])))
    for m, so, p in procs:
        assert p.wait() == 0
        lib = C.CDLL(so)
        lib.emu_sp_keyed.restype = C.c_int
        lib.emu_sp_error.restype = C.c_char_p
        lib.emu_sp_hash.restype = C.c_uint64
        lib.emu_sp_table_bits.restype = lib.emu_sp_tile.restype = lib.emu_sp_passes.restype = lib.emu_sp_mutation.restype = C.c_uint32
        assert lib.emu_sp_mutation() == m
        libs[m] = lib
    return libs


def run(lib, ev, key, grid=3, seed=1, **kw):
    call = lambda i, s, o: lib.emu_sp_keyed(i, s, o, C.c_uint32(grid), C.c_uint64(seed))
    st, got = columns.pair_keyed_events_raw(ev, key, call=call, **kw)
    return st, got, lib.emu_sp_error().decode()


@pytest.mark.parametrize("name", CASES)
def test_emulator_equals_split_events_and_tbc_pair_events(emus, name):
    big = name in S.BIG_CASES
    for i, (ev, key) in enumerate(S.cases()[name]):
        for packed, word in (S.forms(name)[:1] if big else S.forms(name)):
            want = S.reference(name, i, ev, key, word, packed) if not big else dict(zip(("keys", "ev_off", "row_of"), columns.split_events(ev, key)))
            if big:
                want["n_keys"] = len(want["keys"])
            for grid, seed in (((3, 1), (1, 2)) if big else ((3, 1), (1, 2), (3, 3))):
                st, got, err = run(emus[0], S.packed(ev) if packed else ev, key, grid=grid, seed=seed, word=word, pair=not big)
                assert st == 0, err
                S.assert_same(got, want, (name, i, packed, word, grid, seed), paired=not big)


@pytest.mark.parametrize("case, i, times", [("sizes", 8, 1), ("chunk_and_tile_edges", 0, 10), ("sizes", 1, 3000)])
def test_regions_for_a_capacity_used_by_a_smaller_call(emus, case, i, times):
    """the batch form (sp::plan_batch / sp::args_batch): the regions laid out for a capacity, a call of fewer rows with its own tile count
    and table size -- a tile more than the rows, ten times the rows, one row in a few thousand"""
    lib = emus[0]
    lib.emu_sp_keyed_cap.restype = C.c_int
    ev, key = S.cases()[case][i]
    n = len(key)
    cap = n + S.T + 5 if times == 1 else times * n
    want = S.reference(case, i, ev, key, True, True)
    pad = lambda x: np.ascontiguousarray(np.concatenate([x, np.zeros(cap - n, x.dtype)]))
    word, process = S.packed(ev)

    def call(inp, split, out):
        inp._obj.n = n
        return lib.emu_sp_keyed_cap(inp, split, out, C.c_uint32(3), C.c_uint64(5), C.c_uint32(cap))

    st, got = columns.pair_keyed_events_raw((pad(word), pad(process)), pad(np.asarray(key, np.int32)), word=True, call=call)
    assert st == 0, lib.emu_sp_error().decode()
    got["row_of"] = got["row_of"][:n]
    S.assert_same(got, want, (case, i, cap))


def test_the_constants_the_shapes_are_built_on(emus):
    lib = emus[0]
    assert lib.emu_sp_tile() == S.T
    for n in (0, 1, 31, 32, 33, 300, 1 << 20, (1 << 20) + 1, 0xFFFFFFFE):
        assert lib.emu_sp_table_bits(C.c_uint64(n)) == S.table_bits(n), n
    for k in (0, 1, -1, -2 ** 31, 2 ** 31 - 1, 123456789):
        for bits in (6, 10, 33):
            assert lib.emu_sp_hash(C.c_uint32(k & 0xFFFFFFFF), C.c_uint32(bits)) == S.table_hash(k, bits), (k, bits)
    for nk in (0, 1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1):
        assert lib.emu_sp_passes(C.c_uint32(nk)) == S.sort_passes(nk), nk
    assert [S.sort_passes(nk) for nk in (255, 256, 257, 65535, 65536, 65537)] == [1, 1, 2, 2, 2, 3]


def test_keys_cap_exact_and_one_below(emus):
    ev, key = S.cases()["refusal_per_key"][0]
    want = S.reference("refusal_per_key", 0, ev, key, False)
    nk = want["n_keys"]
    st, got, err = run(emus[0], ev, key, keys_cap=nk)
    assert st == 0, err
    S.assert_same(got, want, "keys_cap = n_keys")
    st, got, err = run(emus[0], ev, key, keys_cap=nk - 1)
    assert st == N.ERR_INVALID_ARG and f"{nk} distinct keys" in err
    assert got["n_keys"] == 0 and not got["row_of"].any() and got["n_ops"] == 0 and not got["inv_pos"].any()


def test_ops_cap_one_below_writes_nothing(emus):
    ev, key = S.cases()["semantics"][0]
    want = S.reference("semantics", 0, ev, key, False)
    st, got, err = run(emus[0], ev, key, ops_cap=want["n_ops"] - 1)
    assert st == N.ERR_INVALID_ARG and f"{want['n_ops']} ops survive" in err
    assert not got["row_of"].any() and not got["inv_pos"].any() and not got["f"].any()
    st, got, err = run(emus[0], ev, key, ops_cap=want["n_ops"])
    assert st == 0, err
    S.assert_same(got, want, "ops_cap = n_ops")


def test_split_only_and_row_of_not_wanted(emus):
    ev, key = S.cases()["chunk_and_tile_edges"][0]
    want = S.reference("chunk_and_tile_edges", 0, ev, key, False)
    st, got, err = run(emus[0], ev, key, pair=False)
    assert st == 0, err
    S.assert_same(got, want, "split only", paired=False)
    st, got, err = run(emus[0], ev, key, row_of=False, columns=False)
    assert st == 0 and "row_of" not in got and "f" not in got, err
    S.assert_same(got, {k: v for k, v in want.items() if k not in ("f", "a", "b", "process")}, "no row_of", row_of=False)
    st, got, err = run(emus[0], S.packed(ev), key, pair=False, row_of=False)
    assert st == 0, err
    S.assert_same(got, want, "split only, packed, no row_of", row_of=False, paired=False)


@pytest.mark.parametrize("mutation, seen_by", [(1, "first_appearance_descending"), (2, "two_keys_alternating")])
def test_planted_mutations_are_seen(emus, mutation, seen_by):
    """1: a key's id is its rank by VALUE, not by first appearance; 2: the scatter ranks a row within its tile only (every tile writes from
    the first tile's bases)"""
    ev, key = S.cases()[seen_by][0]
    want = S.reference(seen_by, 0, ev, key, False)
    st, got, err = run(emus[mutation], ev, key)
    assert st == 0, err
    with pytest.raises(AssertionError):
        S.assert_same(got, want, seen_by)
    st, good, err = run(emus[0], ev, key)
    S.assert_same(good, want, seen_by)


def split_alone(lib, ev, key, grid, seed):
    st, got, err = run(lib, ev, key, grid=grid, seed=seed, pair=False)
    assert st == 0, err
    return got


@pytest.mark.parametrize("name, grid, seed", [("top_scan_second_step", 3, 21), ("top_scan_three_passes", 3, 22), ("three_passes_many_rows", 1, 23)])
def test_past_2_to_the_20_rows(emus, name, grid, seed):
    """the large shapes (keyed_events_shapes.large_cases), the split alone, once each: sp_top_kernel's second step of 256 block sums,
    with two and with three passes of the sort, and several rows a key through three passes -- keys, ev_off and row_of bit for bit
    against columns.split_events"""
    ev, key = S.large_cases()[name]
    S.assert_same(split_alone(emus[0], ev, key, grid, seed), S.large_reference(name), (name, grid, seed), paired=False)


def test_the_second_step_of_the_top_scan_is_seen_past_2_to_the_20_rows_alone(emus):
    """mutation 3: sp_top_kernel stores a block's base without what the steps before carried.  The largest history of cases(),
    digit_edges_16[2] (65,537 rows: 17 blocks), PASSES under it -- the gap these shapes close; 2^20 + 1 rows (257 blocks) see it."""
    ev, key = S.cases()["digit_edges_16"][2]
    want = dict(zip(("keys", "ev_off", "row_of"), columns.split_events(ev, key)))
    want["n_keys"] = len(want["keys"])
    S.assert_same(split_alone(emus[3], ev, key, 3, 1), want, "digit_edges_16[2] under mutation 3", paired=False)
    ev, key = S.large_cases()["top_scan_second_step"]
    got = split_alone(emus[3], ev, key, 3, 21)
    with pytest.raises(AssertionError):
        S.assert_same(got, S.large_reference("top_scan_second_step"), "top_scan_second_step under mutation 3", paired=False)


def test_a_probe_that_does_not_wrap_is_seen_by_the_wrapping_case_alone(emus):
    """mutation 4: behind the last slot of the table the probe stays there (in bounds; `t <= mask` ends it) in sp_insert_kernel and
    sp_first_row.  colliding_keys, whose probe runs lie in the middle of the table, passes under it; probe_run_wraps does not.  The
    split alone: the mutated table loses keys, and the pairing is not to run over what is left."""
    for name, seen in (("colliding_keys", False), ("probe_run_wraps", True)):
        ev, key = S.cases()[name][0]
        want = S.reference(name, 0, ev, key, False)
        for grid, seed in ((3, 1), (1, 2)):
            S.assert_same(split_alone(emus[0], ev, key, grid, seed), want, (name, grid, seed), paired=False)
            got = split_alone(emus[4], ev, key, grid, seed)
            if seen:
                with pytest.raises(AssertionError):
                    S.assert_same(got, want, (name, "mutation 4", grid, seed), paired=False)
            else:
                S.assert_same(got, want, (name, "mutation 4", grid, seed), paired=False)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """emu_split.cpp with its own main and the specification of the pairing linked in, built with -fsanitize=address,undefined and run
    as a plain executable (the sanitizers' runtimes are linked into the program itself, so nothing has to be loaded before it): what
    would see a write of the scatter, the gather or the scans outside the arena.  Nothing is loaded into Python under a sanitizer."""
    exe = str(tmp_path / "emu_split")
    subprocess.check_call(FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-DEMU_SPLIT_MAIN",
                                   "-D__host__=", "-D__device__=", SRC, os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc", "tbc_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout + out.stderr

"""The planner of a set-full object (csrc/set_full_plan.h, sf_make_layout) on the CPU: the one function that says where every array of
an object lies in its arena, how every key is chunked and which tile of which grid is whose.  set_full_host.hip builds every object from
it, and the emulator programs of the encoding and of the results call it too; here it is built into a few C functions
(tests/emu/setfull_plan.cpp, g++) and what it returns is held against the properties the kernels rest on.  No number here is measured:
the chunking is test_set_full_timing._chunks (the rule, restated there for the shapes' sake), the rest is alignment and order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_set_full_timing import LONG_SHAPE, MANY_SHAPE, SHAPES, TALL_SHAPE, _chunks

DENSE, ROWS, OPS = 0, 1, 2
FIRST_ROWS, FIRST_PREFIX, FIRST_ANY, FIRST_RESOLVE, FIRST_SELECT, FIRSTS = range(6)
# SfArena's regions, in the arena's order
REGIONS = ("plan", "first", "pmax", "enc", "add_invoke", "add_ok", "read_invoke", "read_ok", "top", "exc_off", "exc", "M", "P", "any", "out",
           "words", "element", "val_lo", "val_hi", "slots", "row_flag", "key_flag", "unknown", "repeats", "cnt", "dup_max", "dup_count")
ROWS_ONLY = {"top", "exc_off", "exc"}
OPS_ONLY = {"enc", "element", "val_lo", "val_hi", "slots", "row_flag", "key_flag", "unknown", "repeats", "cnt", "dup_max", "dup_count"}
UNUSED = {DENSE: ROWS_ONLY | OPS_ONLY, ROWS: OPS_ONLY, OPS: ROWS_ONLY}
# one key; four keys: one without elements, one without reads, and a last one of 1,024 elements = 32 words = 8 resolve workgroups, which
# the planner starts on a multiple of 8 (the three before it take 1 + 0 + 33 = 34 workgroups)
OBJECTS = {"one": [(129, 130)], "four": [(33, 130), (0, 5), (4100, 0), (1024, 2049)]}


class KeyPlan(C.Structure):       # SfKeyPlan
    _fields_ = [(f, C.c_uint32) for f in ("E", "R", "WPR", "PITCH", "rows_per_chunk", "chunks", "elem_base", "row_base", "pmax_off", "any_gy")] + \
               [("m_off", C.c_uint64), ("sum_off", C.c_uint64)]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sf_plan") / "libsetfull_plan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "setfull_plan.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.sfp_regions.restype = lib.sfp_sizeof_key_plan.restype = C.c_uint32
    lib.sfp_make.restype = C.c_int
    assert lib.sfp_regions() == len(REGIONS) and lib.sfp_sizeof_key_plan() == C.sizeof(KeyPlan)
    return lib


def make(lib, keys, source, words_per_row=0, n_exceptions=0):
    """-> the layout of `keys` = [(E, R), ...] as a dict: plan (KeyPlan per key), first [grid][key], tiles, regions {name: (at, bytes)}, ..."""
    n = len(keys)
    E, R = (np.ascontiguousarray([k[i] for k in keys], np.uint32) for i in (0, 1))
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    fits = lib.sfp_make(C.c_uint32(n), u32(E), u32(R), C.c_uint32(source), C.c_uint32(words_per_row), C.c_uint64(n_exceptions))
    plan = (KeyPlan * n)()
    first, tiles = np.zeros(FIRSTS * (n + 1), np.uint32), np.zeros(FIRSTS, np.uint64)
    at, size = np.zeros(len(REGIONS), np.uint64), np.zeros(len(REGIONS), np.uint64)
    enc, totals = np.zeros(2 * n, np.uint64), np.zeros(11, np.uint64)
    lib.sfp_get(plan, u32(first), u64(tiles), u64(at), u64(size), u64(enc), u64(totals))
    out = dict(zip(("bytes", "head_bytes", "enc_zero_bytes", "m_words", "sum_words", "pmax_words", "tab_slots", "bytes_matrix", "sumE", "sumR", "enc_keys"),
                   (int(x) for x in totals)))
    out.update(fits=bool(fits), plan=list(plan), first=first.reshape(FIRSTS, n + 1).astype(np.int64), tiles=[int(t) for t in tiles],
               regions={name: (int(a), int(b)) for name, a, b in zip(REGIONS, at, size)}, enc=enc.reshape(n, 2))
    return out


@pytest.mark.parametrize("E,R", SHAPES + [LONG_SHAPE, MANY_SHAPE, TALL_SHAPE, (0, 130), (129, 0), (0, 0)])
def test_the_chunking_is_the_rule_the_timing_tests_build_their_keys_on(planner, E, R):
    p = make(planner, [(E, R)], ROWS)["plan"][0]
    assert (p.chunks, p.rows_per_chunk) == _chunks(E, R)
    assert p.rows_per_chunk <= 2048 and p.chunks * p.rows_per_chunk >= R           # (kSetFullRows: a chunk's rows are staged in LDS)


@pytest.mark.parametrize("source", (DENSE, ROWS, OPS), ids=("dense", "rows", "ops"))
@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_layout(planner, name, source):
    keys = OBJECTS[name]
    n, sumE, sumR = len(keys), sum(k[0] for k in keys), sum(k[1] for k in keys)
    wpr = max((E + 31) // 32 for E, _ in keys) + 1
    L = make(planner, keys, source, words_per_row=wpr if source == DENSE else 0, n_exceptions=7 if source == ROWS else 0)
    assert L["fits"] and (L["sumE"], L["sumR"]) == (sumE, sumR)
    # ---- the arena: every region on a multiple of 256 B, in ascending order, none reaching into the next; what the source does not use is empty
    end = 0
    for r in REGIONS:
        at, size = L["regions"][r]
        assert at % 256 == 0 and at >= end, r
        end = at + size
        assert (size == 0) == (r in UNUSED[source]), (r, size)
    assert end <= L["bytes"]
    assert L["head_bytes"] == L["regions"]["add_invoke"][0] and L["enc_zero_bytes"] == L["bytes"] - L["regions"]["slots"][0]
    assert L["regions"]["exc"][1] == (7 * 4 if source == ROWS else 0)
    assert L["enc_keys"] == (n if source == OPS else 0) and (L["tab_slots"] > 0) == (source == OPS)
    # ---- the keys: bases key after key, 64-word starts in the matrix and in the summaries, a pitch of whole 16 B
    eb = rb = 0
    for (E, R), p in zip(keys, L["plan"]):
        assert (p.E, p.R, p.elem_base, p.row_base) == (E, R, eb, rb)
        assert p.WPR == (E + 31) // 32 and p.PITCH % 4 == 0 and 0 <= p.PITCH - p.WPR < 4
        assert p.m_off % 64 == 0 and p.sum_off % 64 == 0
        assert (p.chunks, p.rows_per_chunk) == _chunks(E, R)
        eb, rb = eb + E, rb + R
    assert L["m_words"] >= max(p.m_off + p.R * p.PITCH for p in L["plan"])
    assert L["bytes_matrix"] == 4 * sum(R * (wpr if source == DENSE else (E + 31) // 32) for E, R in keys)
    # ---- the grids: every row of first-tiles ascends and ends at its grid's total; the rows' grid is the reads
    for g in range(FIRSTS):
        assert (np.diff(L["first"][g]) >= 0).all() and L["first"][g][n] == L["tiles"][g], g
    assert L["first"][FIRST_ROWS][n] == sumR and list(L["first"][FIRST_ROWS][:n]) == [p.row_base for p in L["plan"]]
    for k, p in enumerate(L["plan"]):            # a key's tiles fit between its first and its successor's
        nb = (p.WPR + 3) // 4
        assert L["first"][FIRST_RESOLVE][k + 1] - L["first"][FIRST_RESOLVE][k] >= nb
        if nb and nb % 8 == 0:
            assert L["first"][FIRST_RESOLVE][k] % 8 == 0, k
        assert L["first"][FIRST_ANY][k + 1] - L["first"][FIRST_ANY][k] == (p.chunks * p.any_gy if p.E and p.R else 0)
    if name == "four":
        assert L["first"][FIRST_RESOLVE][3] == 40 and L["tiles"][FIRST_RESOLVE] == 48          # 34 rounded up to 40
    # ---- Ops: a table per key, a power of two of at least 2 E slots, one after the other
    if source == OPS:
        off = 0
        for (E, _), (tab_off, mask) in zip(keys, L["enc"]):
            cap = int(mask) + 1 if E else 0
            assert int(tab_off) == off and (E == 0 or (cap & (cap - 1) == 0 and 2 * E <= cap < 4 * E))
            off += cap
        assert off == L["tab_slots"]

"""The keyed route without a device: columns.split_events -- the numpy definition of what tbc_pair_keyed_events splits on the device
-- against jepsen/independent.split on dict histories built from the same columns; the shapes of tests/keyed_events_shapes.py hold
what they are there for; the arguments of tbc_pair_keyed_events are held against the rules of its structs BEFORE the device is looked
for, and valid input on a machine without a gfx950 is TBC_ERR_NO_DEVICE: there is no CPU fallback; the struct layouts against the
header."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import keyed_events_shapes as S
import pair_events_shapes as PS
from conftest import ROOT, has_gpu
from jepsen_tigerbeetle_amd import _native as N, columns
from jepsen_tigerbeetle_amd.jepsen import independent

TYPES = {N.INVOKE: "invoke", N.OK: "ok", N.FAIL: "fail", N.INFO: "info"}


def dict_history(ev, key):
    """the history as Jepsen's op maps, every value an independent tuple [k v]; :index is the row"""
    return [{"index": r, "type": TYPES.get(int(ev.type[r]), "unknown"), "process": int(ev.process[r]), "f": int(ev.f[r]),
             "value": independent.tuple_(int(key[r]), (int(ev.a[r]), int(ev.b[r])))} for r in range(len(ev))]


@pytest.mark.parametrize("name", [n for n in sorted(S.cases()) if n not in S.BIG_CASES])
def test_split_events_is_independent_split(name):
    for ev, key in S.cases()[name]:
        keys, ev_off, row_of = columns.split_events(ev, key)
        want_keys, subs = independent.split(dict_history(ev, key))
        assert list(keys) == want_keys and keys.dtype == np.int32 and ev_off.dtype == np.uint64 and row_of.dtype == np.uint32
        assert ev_off[0] == 0 and int(ev_off[-1]) == len(ev) == len(row_of)
        for h, k in enumerate(want_keys):
            rows = row_of[int(ev_off[h]):int(ev_off[h + 1])]
            assert [op["index"] for op in subs[k]] == list(rows), (name, k)
            assert [op["value"] for op in subs[k]] == [(int(ev.a[r]), int(ev.b[r])) for r in rows]


def test_split_events_on_many_keys():
    for ev, key in S.cases()["digit_edges_16"][2:]:
        keys, ev_off, row_of = columns.split_events(ev, key)
        assert np.array_equal(keys, key) and np.array_equal(row_of, np.arange(len(key))) and np.array_equal(ev_off, np.arange(len(key) + 1))
    with pytest.raises(ValueError):
        columns.split_events(PS.H(PS.pairs(4)), np.zeros(3, np.int32))


def test_the_shapes_hold_what_they_are_there_for():
    c, T = S.cases(), S.T
    assert [len(k) for _, k in c["sizes"]] == [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    (ev, key), = c["one_key"]
    assert len(set(key)) == 1 and len(key) > 2 * T
    (ev, key), = c["every_row_its_own_key"]
    assert len(set(key)) == len(key) > T
    assert [len(set(k)) for _, k in c["digit_edges_8"] + c["digit_edges_16"]] == [255, 256, 257, 65535, 65536, 65537]
    assert [S.sort_passes(n) for n in (1, 2, 256, 257, 65536, 65537)] == [0, 1, 1, 2, 2, 3]
    (ev, key), = c["two_keys_alternating"]
    assert len(key) >= 4 * T and set(key[0::2]) == {9} and set(key[1::2]) == {-9}
    ev, key = c["first_appearance_descending"][0]
    keys, _, _ = columns.split_events(ev, key)
    assert list(keys) == sorted(keys, reverse=True) and len(keys) == 12
    assert {S.INT32_MIN, -1, 0, S.INT32_MAX} == set(c["key_values"][0][1]) == set(c["key_values"][1][1])
    (ev, key), = c["colliding_keys"]
    bits = S.table_bits(len(key))
    hashes = sorted(S.table_hash(int(k), bits) for k in set(key))
    assert len(set(key)) == 24 and hashes[:12] == [hashes[0]] * 12 and hashes[12:] == [hashes[0] + 1] * 12
    ev, key = c["chunk_and_tile_edges"][0]
    for r, done in ((63, PS.OK), (T - 1, PS.OK), (2 * T + 63, PS.FAIL), (3 * T - 1, PS.INFO)):
        assert (ev.type[r], ev.type[r + 1], key[r]) == (PS.I, done, key[r + 1]) and ev.process[r] == ev.process[r + 1] and key[r - 1] != key[r]
    ev, key = c["chunk_and_tile_edges"][1]
    own = columns.take_events(ev, np.flatnonzero(key == 9))
    assert (own.type[63], own.process[63], own.type[64], own.process[64]) == (PS.I, 71, PS.OK, 71)
    ev, key = c["refusal_per_key"][0]
    ref = S.reference("refusal_per_key", 0, ev, key, False)
    assert list(ref["status"]) == [0, N.ERR_BAD_HISTORY, 0, N.ERR_UNSUPPORTED, 0, N.ERR_BAD_HISTORY, 0] and list(ref["bad_row"][[1, 5]]) == [20, 0]
    ev, key = c["wire"][0]
    assert list(S.reference("wire", 0, ev, key, True)["status"]) == list(PS.reference("wire", PS.cases()["wire"], True)["status"])
    ev, key = c["semantics"][0]
    ref, flat = S.reference("semantics", 0, ev, key, False), PS.reference("semantics", PS.cases()["semantics"], False)
    for k in ("op_off", "f", "a", "b", "process", "inv_pos", "ret_pos", "n_process"):       # (the keys appear in the order of the histories)
        assert np.array_equal(ref[k], flat[k]), k


def test_the_table_end_and_many_rows_shapes_hold_what_they_are_there_for():
    c, T = S.cases(), S.T
    (ev, key), = c["probe_run_wraps"]
    bits = S.table_bits(len(key))
    assert (len(key), bits) == (300, 10)
    keys, _, _ = columns.split_events(ev, key)
    home = [S.table_hash(int(k), bits) for k in keys]
    assert (home.count(1023), home.count(1022), home.count(0), len(home)) == (8, 8, 4, 20)
    assert home[:6] == [1023, 1022, 0, 1023, 1022, 0]                      # a key of each group in turn
    (ev, key), = c["many_rows_over_passes"]
    keys, ev_off, row_of = columns.split_events(ev, key)
    per_key = np.diff(ev_off.astype(np.int64))
    assert len(key) == 4 * T + 3 and len(keys) == 257 and S.sort_passes(257) == 2 and (per_key.min(), per_key.max()) == (15, 16)
    tiles = [len(set(row_of[int(ev_off[h]):int(ev_off[h + 1])] // T)) for h in range(257)]      # (a key's rows are 257 apart)
    assert min(tiles) == 4 and max(tiles) == 5
    assert list(keys) != sorted(keys) and list(keys) != sorted(keys, reverse=True)
    ref = S.reference("many_rows_over_passes", 0, ev, key, False)
    assert not ref["status"].any() and ref["n_ops"] > 2 * T


def test_the_large_shapes_hold_what_they_are_there_for():
    """(large_case asserts the thresholds itself: the tiles, the scan's blocks, the passes, the rows a key)"""
    assert S.LARGE_GPU_CASES == S.LARGE_CASES + ("tiles_stride",) and set(S.large_cases()) == set(S.LARGE_CASES)
    for name, (ev, key) in S.large_cases().items():
        assert len(ev) == len(key) > (S.T * S.T if name.startswith("top_scan") else 3 * 65537) and key.dtype == np.int32
    # an invocation and its completion in adjacent rows under one key, behind the keys' first rows
    ev, key = S.large_case("top_scan_second_step")
    body = slice(300, len(key) - 1)
    assert np.array_equal(key[body][0::2], key[body][1::2]) and set(ev.type[body][0::2]) == {PS.I} and set(ev.type[body][1::2]) == {PS.OK}
    assert np.array_equal(ev.process[body][0::2], ev.process[body][1::2])


def test_the_quick_reference_is_the_reference():
    """keyed_events_shapes._all_keys_fine (tbc_pair_events key by key without an array per key) gives what pair_events_shapes.reference gives"""
    for name, i in (("sizes", 8), ("semantics", 0), ("key_values", 0)):
        ev, key = S.cases()[name][i]
        keys, ev_off, row_of = columns.split_events(ev, key)
        moved, off = columns.take_events(ev, row_of), ev_off.astype(np.int64)
        quick = S._all_keys_fine(moved, off, True)
        evs = [columns.take_events(moved, np.arange(off[h], off[h + 1])) for h in range(len(keys))]
        PS.assert_same(quick, PS.reference(("slow", name, i), evs, True), name)
    ev, key = S.cases()["refusal_per_key"][0]
    keys, ev_off, row_of = columns.split_events(ev, key)
    assert S._all_keys_fine(columns.take_events(ev, row_of), ev_off.astype(np.int64), False) is None


def structs(ev, key, keys_cap=None, packed=False):
    n = len(key)
    keep = {"key": np.ascontiguousarray(key, np.int32), "keys": np.zeros(max(n, 1), np.int32), "ev_off": np.zeros(n + 1, np.uint64),
            "word": columns.pack_events(ev) if packed else None}
    p = columns._p
    i = N.KeyedEvents()
    i.n, i.device, i.key, i.process = n, 0, p(keep["key"], C.c_int32), p(ev.process, C.c_int32)
    if packed:
        i.ev_word = p(keep["word"], C.c_uint32)
    else:
        i.type, i.f, i.a, i.b = p(ev.type, C.c_uint8), p(ev.f, C.c_uint8), p(ev.a, C.c_int32), p(ev.b, C.c_int32)
    s = N.SplitOut()
    s.keys_cap, s.keys, s.ev_off = n if keys_cap is None else keys_cap, p(keep["keys"], C.c_int32), p(keep["ev_off"], C.c_uint64)
    _, o, keep2 = PS.structs(np.zeros(n + 1, np.uint64), ev, n, {"inv_pos": np.zeros(max(n, 1), np.uint32), "ret_pos": np.zeros(max(n, 1), np.uint32)})
    return i, s, o, (keep, keep2)


def call(native, i, s, o):
    ref = lambda x: C.byref(x) if x is not None else None
    st = native.lib().tbc_pair_keyed_events(ref(i), ref(s), ref(o))
    return st, native.lib().tbc_last_error().decode()


def test_arguments_are_validated_first(native):
    ev, key = S.cases()["semantics"][0]
    i, s, o, keep = structs(ev, key)
    assert call(native, None, s, o)[0] == N.ERR_INVALID_ARG and call(native, i, None, o)[0] == N.ERR_INVALID_ARG
    for field in ("key", "process", "type", "f", "a", "b"):
        i, s, o, keep = structs(ev, key)
        setattr(i, field, None)
        st, err = call(native, i, s, o)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    i, s, o, keep = structs(ev, key, packed=True)
    i.process = None
    assert call(native, i, s, o)[0] == N.ERR_INVALID_ARG
    for field in ("keys", "ev_off"):
        i, s, o, keep = structs(ev, key)
        setattr(s, field, None)
        st, err = call(native, i, s, None)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    for field in ("op_off", "n_events", "n_process", "status", "bad_row", "inv_pos", "ret_pos"):
        i, s, o, keep = structs(ev, key)
        setattr(o, field, None)
        st, err = call(native, i, s, o)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    # the size alone decides this: no row is looked at
    i, s, o, keep = structs(ev, key)
    i.n = 0xFFFFFFFF
    st, err = call(native, i, s, o)
    assert st == N.ERR_INVALID_ARG and "2^32 - 2 rows" in err


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback(native):
    ev, key = S.cases()["semantics"][0]
    for packed in (False, True):
        i, s, o, keep = structs(ev, key, packed=packed)
        assert call(native, i, s, o)[0] == N.ERR_NO_DEVICE and call(native, i, s, None)[0] == N.ERR_NO_DEVICE
    with pytest.raises(N.NoDeviceError):
        columns.pair_keyed_events(ev, key)
    i, s, o, keep = structs(*S.cases()["sizes"][0])
    assert call(native, i, s, o)[0] == N.ERR_NO_DEVICE


def test_struct_layouts_match_header(native):
    prog = r'''
#include <stdio.h>
#include "tbcheck.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tbc_keyed_events), offsetof(tbc_keyed_events, key),
  offsetof(tbc_keyed_events, ev_word), offsetof(tbc_keyed_events, process), offsetof(tbc_keyed_events, type), offsetof(tbc_keyed_events, b),
  sizeof(tbc_split_out), offsetof(tbc_split_out, n_keys), offsetof(tbc_split_out, keys), offsetof(tbc_split_out, row_of));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tbc_batch_keyed_events), offsetof(tbc_batch_keyed_events, events_cap),
  offsetof(tbc_batch_keyed_events, key), offsetof(tbc_batch_keyed_events, process), sizeof(tbc_keyed_report), offsetof(tbc_keyed_report, n_bad),
  offsetof(tbc_keyed_report, bytes_in), offsetof(tbc_keyed_report, n_keys), offsetof(tbc_keyed_report, row_of)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    K, P, B, R = N.KeyedEvents, N.SplitOut, N.BatchKeyedEvents, N.KeyedReport
    assert sizes == [C.sizeof(K), K.key.offset, K.ev_word.offset, K.process.offset, K.type.offset, K.b.offset, C.sizeof(P), P.n_keys.offset,
                     P.keys.offset, P.row_of.offset, C.sizeof(B), B.events_cap.offset, B.key.offset, B.process.offset, C.sizeof(R),
                     R.n_bad.offset, R.bytes_in.offset, R.n_keys.offset, R.row_of.offset]
    # tbc_keyed_report begins as tbc_events_report does: the library fills the shared fields through one function
    E = N.EventsReport
    assert all(getattr(R, f).offset == getattr(E, f).offset for f, _ in E._fields_)
    assert native.lib().tbc_version() == 2

"""The packed event word on the host, no device needed: tbc_pack_events against the numpy statement of TBC_EVENT_WORD
(tests/packed_events_shapes.py) on every shape and every field edge; the new structs against the header; tbc_pair_packed_batch's
arguments held against the rules BEFORE the device is looked for, then TBC_ERR_NO_DEVICE (no CPU fallback); the batch entry points
refuse a null batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import packed_events_shapes as P
import pair_events_shapes as S
from conftest import ROOT, has_gpu
from jepsen_tigerbeetle_amd import _native as N, columns

CASES = sorted(P.cases())


@pytest.mark.parametrize("name", CASES)
def test_pack_equals_the_numpy_statement(native, name):
    for h, e in enumerate(P.cases()[name]):
        got = columns.pack_events(e)
        assert got.dtype == np.uint32 and np.array_equal(got, P.pack(e)), (name, h)


def test_pack_random_batch(native):
    for h, e in enumerate(S.random_batch()):
        w = columns.pack_events(e)
        assert np.array_equal(w, P.pack(e)), h
        d = P.decode(w, e.process)          # such histories hold nothing the word does not: they come back as they went
        for k in ("type", "process", "f", "a", "b"):
            assert np.array_equal(getattr(d, k), getattr(e, k)), (h, k)


def test_every_field_edge(native):
    word = lambda t, f, a, b: int(columns.pack_events(S.H([(t, 0, f, a, b)]))[0])
    W = lambda t, f, a, b: t | f << 3 | a << 8 | b << 17
    for t, code in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 7), (7, 7), (255, 7)):
        assert word(t, 1, 2, 3) == W(code, 1, 2, 3), t
    for f, code in ((0, 0), (15, 15), (16, 16), (17, 16), (255, 16)):
        assert word(0, f, 2, 3) == W(0, code, 2, 3), f
    for v, code in ((0, 0), (254, 254), (255, 256), (256, 256), (-1, 256), (2 ** 31 - 1, 256), (-2 ** 31 + 1, 256), (N.NIL, 255)):
        assert word(1, 2, v, 0) == W(1, 2, code, 0), v
        assert word(1, 2, 0, v) == W(1, 2, 0, code), v
    assert word(255, 255, -1, -1) == W(7, 16, 256, 256) < 1 << 26
    assert (N.EVW_TYPE_UNKNOWN, N.EVW_F_ABOVE, N.EVW_NIL, N.EVW_UNFIT) == (P.TYPE_UNKNOWN, P.F_ABOVE, P.V_NIL, P.V_UNFIT)
    # the decoded history is decided as the original is: the reference of the packed form against the reference of the columns
    for name in ("wire", "malformed_each", "bad_among_good", "semantics"):
        evs = S.cases()[name]
        a, b = P.packed_reference(name, evs), S.reference(name, evs, True)
        for k in ("status", "bad_row", "op_off", "n_process", "inv_pos", "ret_pos", "word"):
            assert np.array_equal(a[k], b[k]), (name, k)


def test_pack_arguments(native):
    lib = native.lib()
    e = S.H(S.pairs(4))
    es = e.struct()
    assert lib.tbc_pack_events(None, None) == N.ERR_INVALID_ARG
    assert lib.tbc_pack_events(C.byref(es), None) == N.ERR_INVALID_ARG and "null argument" in lib.tbc_last_error().decode()
    es.a = None
    out = np.zeros(4, np.uint32)
    assert lib.tbc_pack_events(C.byref(es), columns._p(out, C.c_uint32)) == N.ERR_INVALID_ARG
    empty = S.H([]).struct()
    assert lib.tbc_pack_events(C.byref(empty), None) == 0
    with pytest.raises(ValueError):
        columns.pack_events(e, out=np.zeros(3, np.uint32))
    into = np.full(6, 0xA5A5A5A5, np.uint32)
    columns.pack_events(e, out=into[1:5])
    assert into[0] == into[5] == 0xA5A5A5A5 and np.array_equal(into[1:5], P.pack(e))


def structs(ev_off, words, process, ops_cap):
    n = max(int(ev_off[-1]), 1)
    i, o, keep = S.structs(ev_off, S.H(S.pairs(2)), ops_cap, {"inv_pos": np.zeros(n, np.uint32), "ret_pos": np.zeros(n, np.uint32)})
    p = N.PackedEventBatch()
    p.n_hist, p.device, p.ev_off = len(ev_off) - 1, 0, columns._p(ev_off, C.c_uint64)
    p.ev_word, p.process = columns._p(words, C.c_uint32), columns._p(process, C.c_int32)
    return p, o, (keep, ev_off, words, process)


def call(native, i, o):
    st = native.lib().tbc_pair_packed_batch(C.byref(i) if i is not None else None, C.byref(o) if o is not None else None)
    return st, native.lib().tbc_last_error().decode()


def test_packed_batch_arguments_are_validated_first(native):
    make = lambda: structs(*P.concat_packed(S.cases()["semantics"]), ops_cap=100)
    assert call(native, None, None)[0] == N.ERR_INVALID_ARG
    i, o, keep = make()
    assert call(native, i, None)[0] == N.ERR_INVALID_ARG and call(native, None, o)[0] == N.ERR_INVALID_ARG
    for field in ("ev_off", "ev_word", "process"):
        i, o, keep = make()
        setattr(i, field, None)
        st, err = call(native, i, o)
        assert st == N.ERR_INVALID_ARG and "tbc_pair_packed_batch" in err and "null argument" in err, (field, err)
    for field in ("op_off", "n_events", "n_process", "status", "bad_row", "inv_pos", "ret_pos"):
        i, o, keep = make()
        setattr(o, field, None)
        st, err = call(native, i, o)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    i, o, keep = make()
    keep[1][0] = 1
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "ev_off[0]" in err
    i, o, keep = make()
    keep[1][3] = keep[1][2] - 1
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "history 2" in err and "descends" in err
    i, o, keep = make()
    keep[1][1:] += np.uint64(1 << 31)
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "history 0 has 2^31 events" in err
    i, o, keep = make()
    keep[1][1:] = (np.arange(1, len(keep[1])) * ((1 << 31) - 1)).astype(np.uint64)
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "2^32 - 1 events" in err


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback(native):
    i, o, keep = structs(*P.concat_packed(S.cases()["semantics"]), ops_cap=100)
    assert call(native, i, o)[0] == N.ERR_NO_DEVICE
    i, o, keep = structs(*P.concat_packed([]), ops_cap=0)
    assert call(native, i, o)[0] == N.ERR_NO_DEVICE


def test_batch_entry_points_refuse_a_null_batch(native):
    lib = native.lib()
    m, r = N.BatchEvents(), N.EventsReport()
    assert lib.tbc_batch_map_events(None, 0, 0, C.byref(m)) == N.ERR_INVALID_ARG and "tbc_batch_map_events" in lib.tbc_last_error().decode()
    assert lib.tbc_batch_submit_events(None, 0, 1, C.byref(r)) == N.ERR_INVALID_ARG and "tbc_batch_submit_events" in lib.tbc_last_error().decode()
    assert lib.tbc_batch_submit_events(None, 0, 1, None) == N.ERR_INVALID_ARG


def test_struct_layouts_match_header(native, tmp_path):
    structs_ = {"tbc_packed_event_batch": N.PackedEventBatch, "tbc_batch_events": N.BatchEvents, "tbc_events_report": N.EventsReport}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tbcheck.h"', "int main(void){"]
    for name, cls in structs_.items():
        lines.append('printf("%%zu", sizeof(%s));' % name)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (name, f) for f, _ in cls._fields_]
        lines.append('printf("\\n");')
    lines.append('printf("%u %u %u %u %u %llu\\n", TBC_EVW_TYPE_UNKNOWN, TBC_EVW_F_ABOVE, TBC_EVW_NIL, TBC_EVW_UNFIT, TBC_EVENT_WORD(3, 15, 254, 255), TBC_EVENTS_DESC_BYTES(7));')
    lines.append("return 0; }")
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for (name, cls), row in zip(structs_.items(), rows):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_] == row, name
    assert rows[3] == [7, 16, 255, 256, int(P.event_word(3, 15, 254, 255)), N.events_desc_bytes(7)] and N.events_desc_bytes(7) == P.descriptor_bytes(7)
    for name in ("tbc_pack_events", "tbc_pair_packed_batch", "tbc_batch_map_events", "tbc_batch_submit_events"):
        assert name in N.SYMBOLS and hasattr(native.lib(), name)
    assert native.lib().tbc_version() == 2

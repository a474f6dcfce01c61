"""The history as op columns (tbc_setfull_keys_create_ops, include/tbcheck.h), the part that needs no GPU: the new symbols and the two
structs' layout against the header, every rule of the input refused on the host with the key and the op named, no CPU fallback,
`OpColumns` (a plain copy: nemesis ops dropped, non-integer values refused), and the merge of the library's dup_max with the duplicates
among unknown values on hand-made encodings."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from helpers import set_history
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import set_full as sf
from test_set_full_encode_emu import HAND, _h, ops_in


def test_symbols_and_struct_layouts_match_header(native):
    for name in ("tbc_setfull_keys_create_ops", "tbc_setfull_keys_shape", "tbc_setfull_keys_encoding"):
        assert name in native.SYMBOLS and hasattr(native.lib(), name)
    I, O = native.SetFullOpsIn, native.SetFullEncoding
    fi, fo = [f for f, _ in I._fields_], [f for f, _ in O._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tbcheck.h"\nint main(void){ printf("%zu", sizeof(tbc_setfull_ops_in));\n'
    prog += "".join('printf(" %%zu", offsetof(tbc_setfull_ops_in, %s));\n' % f for f in fi)
    prog += 'printf(" %zu", sizeof(tbc_setfull_encoding));\n'
    prog += "".join('printf(" %%zu", offsetof(tbc_setfull_encoding, %s));\n' % f for f in fo)
    prog += 'printf(" %u %u %u %u", TBC_SETFULL_T_INVOKE, TBC_SETFULL_T_OK, TBC_SETFULL_T_FAIL, TBC_SETFULL_T_INFO);\n'
    prog += 'printf(" %u %u %u %u %u %u\\n", TBC_SETFULL_T_NIL, TBC_SETFULL_OP_OTHER, TBC_SETFULL_OP_ADD, TBC_SETFULL_OP_READ, TBC_SETFULL_ENCODE_WINDOW_WORDS, TBC_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    mine = [C.sizeof(I)] + [getattr(I, f).offset for f in fi] + [C.sizeof(O)] + [getattr(O, f).offset for f in fo]
    mine += [N.SETFULL_T_INVOKE, N.SETFULL_T_OK, N.SETFULL_T_FAIL, N.SETFULL_T_INFO, N.SETFULL_T_NIL, N.SETFULL_OP_OTHER, N.SETFULL_OP_ADD,
             N.SETFULL_OP_READ, N.SETFULL_ENCODE_WINDOW_WORDS, 2]
    assert mine == got
    assert C.sizeof(I) == 72 and C.sizeof(O) == 88


def _status(s):
    h = C.c_void_p()
    st = N.lib().tbc_setfull_keys_create_ops(C.byref(s), C.byref(h))
    if st == 0:
        N.lib().tbc_setfull_keys_destroy(h)
    return st, N.lib().tbc_last_error().decode()


def _two_keys():
    """key 0: 12 ops, key 1: 7 ops (two reads with values)"""
    return sf.OpColumns.of_keys({"a": HAND["re-added"], "b": HAND["fail-read"]})


def test_every_rule_is_refused_on_the_host_naming_key_and_op(native):
    fn = "tbc_setfull_keys_create_ops"
    # a null pointer, each in turn
    for f in ("op_off", "index", "type", "f", "process", "value", "val_off", "vals"):
        s, keep = ops_in(_two_keys())
        setattr(s, f, None)
        st, msg = _status(s)
        assert st == N.ERR_INVALID_ARG and fn in msg and "null" in msg, (f, msg)
    assert N.lib().tbc_setfull_keys_create_ops(None, None) == N.ERR_INVALID_ARG
    s, keep = ops_in(_two_keys())
    s.n_keys = 0
    st, msg = _status(s)
    assert st == N.ERR_INVALID_ARG and "n_keys" in msg

    def broken(change):
        s, keep = ops_in(_two_keys())
        change(keep)
        return _status(s)

    # op_off descending
    st, msg = broken(lambda k: k["op_off"].__setitem__(1, 30))
    assert st == N.ERR_INVALID_ARG and fn in msg and "key 1" in msg and "op_off" in msg, msg
    # index not strictly ascending inside key 1 (its op 3 repeats op 2's index); the first op of a key may number below the key before
    st, msg = broken(lambda k: k["index"].__setitem__(12 + 3, k["index"][12 + 2]))
    assert st == N.ERR_INVALID_ARG and fn in msg and "key 1 op 3" in msg and "index" in msg, msg
    st, msg = broken(lambda k: k["index"].__setitem__(5, 0xFFFFFFFF))
    assert st == N.ERR_INVALID_ARG and "key 0 op 5" in msg, msg
    # val_off: not from 0; descending at key 1's op 6 (the read that has a value)
    st, msg = broken(lambda k: k["val_off"].__setitem__(0, 1))
    assert st == N.ERR_INVALID_ARG and fn in msg and "val_off[0]" in msg, msg
    st, msg = broken(lambda k: k["val_off"].__setitem__(12 + 6 + 1, 0))
    assert st == N.ERR_INVALID_ARG and "key 1 op 6" in msg and "val_off" in msg, msg
    # type and f out of range (TBC_SETFULL_T_NIL or-ed in is in range)
    st, msg = broken(lambda k: k["type"].__setitem__(4, 4))
    assert st == N.ERR_INVALID_ARG and "key 0 op 4" in msg and "type" in msg, msg
    st, msg = broken(lambda k: k["type"].__setitem__(12, 0x40))
    assert st == N.ERR_INVALID_ARG and "key 1 op 0" in msg and "type" in msg, msg
    st, msg = broken(lambda k: k["f"].__setitem__(11, 3))
    assert st == N.ERR_INVALID_ARG and "key 0 op 11" in msg and "(index 11)" in msg and "f is not" in msg, msg
    # ... and valid input gets as far as the device: there is no CPU fallback
    st, msg = broken(lambda k: k["type"].__setitem__(2, k["type"][2] | N.SETFULL_T_NIL))
    assert st == (N.OK_STATUS if has_gpu() else N.ERR_NO_DEVICE), msg
    st, msg = _status(ops_in(_two_keys())[0])
    assert st == (N.OK_STATUS if has_gpu() else N.ERR_NO_DEVICE), msg
    h, e, a, b = C.c_void_p(), N.SetFullEncoding(), C.c_uint64(), C.c_uint64()
    assert N.lib().tbc_setfull_keys_encoding(None, C.byref(e)) == N.ERR_INVALID_ARG
    assert N.lib().tbc_setfull_keys_shape(None, C.byref(a), C.byref(b)) == N.ERR_INVALID_ARG


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_column_paths_have_no_cpu_fallback(native):
    hists = {k: set_history(100, 3, k) for k in range(3)}
    with pytest.raises(N.NoDeviceError):
        sf.check_keys_columns(hists, True)
    with pytest.raises(N.NoDeviceError):
        sf.check_columns(hists[0])
    with pytest.raises(N.NoDeviceError):
        sf.KeyedScan.from_ops(sf.OpColumns(hists[1]))
    assert sf.check_keys_columns({}) == {}


def test_op_columns_is_a_plain_copy():
    h = set_history(200, 4, 3, info=0.1)
    nem = {"type": "info", "f": "start-partition", "value": None, "process": "nemesis"}
    mixed = [nem] + h[:50] + [dict(nem, f="stop-partition")] + h[50:]
    c = sf.OpColumns(mixed)
    client = [(i, o) for i, o in enumerate(mixed) if isinstance(o["process"], int)]
    assert len(c.index) == len(h) == len(client) and c.keys == [0] and c.op_off.tolist() == [0, len(h)]
    assert c.index.tolist() == [i for i, _ in client]                            # numbered by position in the WHOLE history
    assert c.n_ops == [len(mixed)] and c.op_time == [None] and c.unit == [1]
    code = {"invoke": 0, "ok": 1, "fail": 2, "info": 3}
    for row, (i, o) in enumerate(client):
        assert c.f[row] == {"add": N.SETFULL_OP_ADD, "read": N.SETFULL_OP_READ}[o["f"]] and c.process[row] == o["process"]
        nil = o["f"] == "read" and o["type"] == "ok" and o["value"] is None
        assert c.type[row] == code[o["type"]] | (N.SETFULL_T_NIL if nil else 0)
        vals = c.vals[int(c.val_off[row]):int(c.val_off[row + 1])].tolist()
        if o["f"] == "add":
            assert c.value[row] == o["value"] and vals == []
        else:
            assert vals == (o["value"] if o["type"] == "ok" and o["value"] else [])
    assert c.n_add_invokes == [sum(o["f"] == "add" and o["type"] == "invoke" for o in h)]
    assert c.n_ok_reads == [sum(o["f"] == "read" and o["type"] == "ok" and o["value"] is not None for o in h)]
    # no set-full semantics: an :ok read without an invocation and a value nobody added are copied like any other
    c = sf.OpColumns(HAND["ok-read-without-invocation"])
    assert c.vals.tolist() == [1, 1, 1, 77, 77] and c.val_off.tolist() == [0, 0, 0, 2, 2, 2, 2, 5]
    # other :f and unknown :type are OTHER; time columns as Encoded keeps them
    t = [dict(o, time=1000 * i) for i, o in enumerate(h)]
    c = sf.OpColumns.of_keys({"x": t, "y": t[:10] + [{k: v for k, v in t[10].items() if k != "time"}] + t[11:20], "z": []})
    e = sf.Encoded(t), sf.Encoded(t[:10] + [{k: v for k, v in t[10].items() if k != "time"}] + t[11:20])
    assert c.unit == [1_000_000, 1, 1] and c.n_ops == [len(t), 20, 0] and c.op_time[2] is None
    assert np.array_equal(c.op_time[0], e[0].op_time) and np.array_equal(c.op_time[1], e[1].op_time)
    c = sf.OpColumns([{"type": "invoke", "f": "txn", "value": [1], "process": 0}, {"type": "sleep", "f": "add", "value": "x", "process": 0}])
    assert c.f.tolist() == [N.SETFULL_OP_OTHER] * 2
    # take: the keys at some positions as columns of their own
    three = sf.OpColumns.of_keys({"a": HAND["re-added"], "b": HAND["fail-read"], "c": HAND["empty-read"]})
    two = three.take([2, 0])
    want = sf.OpColumns.of_keys({"c": HAND["empty-read"], "a": HAND["re-added"]})
    for f in ("op_off", "index", "type", "f", "process", "value", "val_off", "vals"):
        assert np.array_equal(getattr(two, f), getattr(want, f)), f
    assert two.keys == ["c", "a"] and two.n_ops == want.n_ops


@pytest.mark.parametrize("bad", ("x", 1.5, None, True, 2 ** 63, [1]))
def test_op_columns_refuses_what_is_not_an_int64(bad):
    with pytest.raises(ValueError):
        sf.OpColumns(_h([("invoke", "add", bad, 0)]))
    if bad is not None and bad is not True and not isinstance(bad, list):
        with pytest.raises(ValueError):
            sf.OpColumns(_h([("invoke", "read", None, 0), ("ok", "read", [1, bad], 0)]))
    sf.OpColumns(_h([("invoke", "add", -2 ** 63, 0), ("ok", "read", [2 ** 63 - 1, -2 ** 63], 0)]))


def test_duplicates_merge_on_hand_made_encodings():
    """What check_keys_columns makes of tbc_setfull_encoding's dup_max and unknown_values, without a device: the encoding written by hand
    as the library would return it (tests/test_set_full_encode_emu.py has the kernels' side), against Encoded.duplicated."""
    u32 = lambda *x: np.array(x, np.uint32)
    # a duplicated element: 7 three times in one read, twice in another; no unknown values, so the values are never looked at
    h = _h([("invoke", "add", 7, 0), ("ok", "add", 7, 0), ("invoke", "add", 9, 0), ("invoke", "read", None, 1), ("ok", "read", [7, 9, 7], 1),
            ("invoke", "read", None, 1), ("ok", "read", [7, 7, 9, 7], 1)])
    cols = sf.OpColumns.of_keys({"k": h})
    got = sf.duplicated_of_key(cols, 0, np.array([7, 9]), u32(3, 0), 0, u32(4, 6))
    assert got == sf.Encoded(h).duplicated == {7: 3}
    cols.vals = None                                      # (not touched when the key has no unknown value)
    assert sf.duplicated_of_key(cols, 0, np.array([7, 9]), u32(3, 0), 0, u32(4, 6)) == {7: 3}
    # a duplicated unknown value next to a duplicated element, in the second of two keys; a read without an invocation does not count
    g = _h([("invoke", "add", 1, 0), ("ok", "read", [50, 50, 50, 50], 3), ("invoke", "read", None, 1), ("ok", "read", [50, 1, 50, 60], 1),
            ("invoke", "read", None, 2), ("invoke", "read", None, 1), ("ok", "read", [60, 1, 1, 60, 50, 60], 1), ("ok", "read", [70], 2)])
    cols = sf.OpColumns.of_keys({"k": h, "g": g})
    enc = sf.Encoded(g)
    assert enc.read_ok.tolist() == [3, 7, 6] and enc.duplicated == {50: 2, 60: 3, 1: 2}
    got = sf.duplicated_of_key(cols, 1, np.array([1]), u32(2), 7, enc.read_ok)
    assert got == enc.duplicated
    assert sf.unknown_duplicates(cols, 1, np.array([1]), enc.read_ok) == {50: 2, 60: 3}
    assert sf.unknown_duplicates(cols, 0, np.array([7, 9]), u32(4, 6)) == {}
    # the verdict: any duplicate makes the result false, whatever the device's summary says
    dev = {"outcome": np.array([N.SETFULL_STABLE], np.uint8), "stable_latency": np.zeros(1, np.int64),
           "summary": {"valid": True, "attempt_count": 1, "stable_count": 1, "lost_count": 0, "never_read_count": 0, "stale_count": 0,
                       "stable_q": [0] * 5, "lost_q": None, "worst": []}}
    r = sf.result_from_device(sf._Named([1], got), dev)
    assert r["valid?"] is False and r["duplicated"] == {1: 2, 50: 2, 60: 3} and r["duplicated-count"] == 3
    assert sf.result_from_device(sf._Named([1], {}), dev)["valid?"] is True

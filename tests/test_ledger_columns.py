"""jepsen/ledger.py LedgerColumns against the history, field by field, and its ValueErrors; every TBC_ERR_INVALID_ARG rule of
tbc_ledger_check with its message (the rules are checked on the host before any device call, so they answer on a machine without a GPU),
TBC_ERR_NO_DEVICE for valid input there; and the host plan (csrc/ledger_plan.h) in its stand-alone program, tests/emu/ledger_plan.cpp,
built with -fsanitize=address,undefined."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L
from ledger_histories import Builder, r_mop, random_ledger, t_mop


def test_columns_field_by_field():
    h, opts = random_ledger(5, workers=3, transfers=90, reads=15, info=0.1, fail=0.1, plant=("nil", "unexpected", "dup-id"))   # (lookups of 64 and more micro-ops go in as one array)
    h.insert(7, {"type": "invoke", "f": "txn", "value": [], "process": 1, "index": -1})             # no first micro-op: OTHER
    h.insert(8, {"type": "ok", "f": "txn", "value": None, "process": 1, "index": -1})
    cols = L.LedgerColumns(h, opts["total-amount"])
    client = [(i, op) for i, op in enumerate(h) if isinstance(op["process"], int)]
    assert len(cols) == len(client) < len(h)
    assert cols.index.tolist() == [i for i, _ in client] and cols.index.dtype == np.uint32
    assert cols.mop_off[0] == 0 and len(cols.mop_off) == len(cols) + 1 and cols.mop_off[-1] == len(cols.mop_id)
    kinds = set()
    for row, (i, op) in enumerate(client):
        lo, hi = int(cols.mop_off[row]), int(cols.mop_off[row + 1])
        t, k = cols.type[row], cols.kind[row]
        assert t == {"invoke": 0, "ok": 1, "fail": 2, "info": 3}[op["type"]]
        f = op["value"][0][0] if op["value"] else None
        assert k == {"t": N.LEDGER_K_TRANSFER, "r": N.LEDGER_K_READ, "l-t": N.LEDGER_K_LOOKUP, None: N.LEDGER_K_OTHER}[f]
        assert cols.flags[row] == (N.LEDGER_F_FINAL if op.get("final?") else 0)
        kinds.add((int(t), int(k)))
        got = list(zip(cols.mop_id[lo:hi].tolist(), cols.mop_a[lo:hi].tolist(), cols.mop_b[lo:hi].tolist(), cols.mop_c[lo:hi].tolist(), cols.mop_flags[lo:hi].tolist()))
        if op["type"] == "ok" and f == "r":
            want = {}
            for _, ident, m in op["value"]:                                   # the last micro-op of an id wins, in the first one's place
                want[ident] = (ident, m["credits-posted"], m["debits-posted"], 0, 0) if m else (ident, 0, 0, 0, N.LEDGER_M_NIL)
            assert got == list(want.values())
        elif (op["type"] == "invoke" and f == "t") or (op["type"] == "ok" and f == "l-t"):
            assert got == [(ident, m["debit-acct"], m["credit-acct"], m["amount"], 0) for _, ident, m in op["value"]]
        else:
            assert got == []                                                  # (ops no checker looks at keep their kind and no micro-ops)
    assert {(0, 1), (1, 2), (1, 3), (3, 1), (2, 2), (0, 0), (1, 0)} <= kinds
    ok_reads = [i for i, op in client if op["type"] == "ok" and op["value"] and op["value"][0][0] == "r"]
    assert cols.read_ops.tolist() == ok_reads
    assert cols.final_read_ops.tolist() == [i for i in ok_reads if h[i].get("final?")] and len(cols.final_read_ops) == 3
    assert cols.final_lookup_ops.tolist() == [i for i, op in client if op["type"] == "ok" and op["value"] and op["value"][0][0] == "l-t" and op.get("final?")]
    assert any(len({m[1] for m in h[i]["value"]}) < len(h[i]["value"]) for i in ok_reads)          # the planted repeated id is there


def test_columns_value_errors():
    def one(value, type_="ok", final=False, total=0):
        b = Builder()
        b.op(type_, value, 0, final)
        return L.LedgerColumns(b.h, total)

    one([r_mop(1, 2 ** 62, 0)])
    for bad in ([r_mop(1, 2 ** 63, 0)], [r_mop(1, 1.5, 0)], [r_mop(1, True, 0)], [r_mop("a", 1, 0)], [r_mop(None, 1, 0)], [r_mop(-2 ** 63 - 1, 1, 0)],
                [["r", 1, {"credits-posted": 1}]], [["r", 1, {"credits-posted": 1, "debits-posted": 1, "flags": 0}]],
                [["l-t", None, None]], [t_mop("l-t", 1, 1, 2, 2 ** 64)], [["l-t", 1, {"debit-acct": 1, "credit-acct": 2, "amount": 1, "timestamp": 5}]]):
        with pytest.raises(ValueError, match="op 0"):
            one(bad)
    with pytest.raises(ValueError):
        one([t_mop("t", 1, None, 2, 3)], "invoke")
    for bad in (t_mop("l-t", 1, 1, 2, 2 ** 64), t_mop("l-t", 1, 1, 2, True), ["l-t", 1, None][:2] + [{"debit-acct": 1, "credit-acct": 2}], t_mop("l-t", 1.0, 1, 2, 3)):
        with pytest.raises(ValueError, match="op 0"):                         # (the same in a long lookup)
            one([t_mop("l-t", 9, 1, 2, 3)] * 70 + [bad])
    assert len(one([t_mop("l-t", 9, 1, 2, 3)] * 70 + [["l-t", 4, None]]).mop_id) == 71
    one([["l-t", None, None]], "invoke")                                      # (an invoked lookup's micro-ops are not copied)
    # a read whose |credits| + |debits| + |total-amount| reaches 2^63 could wrap a device sum
    one([r_mop(1, 2 ** 62, 2 ** 61), r_mop(2, 2 ** 61 - 1, 0)])
    with pytest.raises(ValueError, match="2\\^63"):
        one([r_mop(1, 2 ** 62, 2 ** 61), r_mop(2, 2 ** 61, 0)])
    with pytest.raises(ValueError, match="2\\^63"):
        one([r_mop(1, 2 ** 62, 0)], total=-2 ** 62)
    with pytest.raises(ValueError, match="2\\^63"):
        one([r_mop(1, -2 ** 62, 2 ** 62)])
    one([r_mop(1, 5, 0), r_mop(1, 6, 0)])                                     # a repeated id: the last wins ...
    with pytest.raises(ValueError, match="twice"):
        one([r_mop(1, 5, 0), r_mop(1, 6, 0)], final=True)                     # ... but a :final? read is compared as a vector
    with pytest.raises(ValueError):
        L.LedgerColumns([], total_amount=2 ** 63)
    # the composed device route has no other route behind it: what the columns refuse, it refuses
    b = Builder()
    b.read([r_mop(1, 5, 0), r_mop(1, 6, 0)], final=True)
    t = L.test({"accounts": [1], "total-amount": 6})
    with pytest.raises(ValueError, match="twice"):
        t["checker"].check(t, b.h)


def valid_columns():
    h, opts = random_ledger(3, transfers=12, reads=9)
    return L.LedgerColumns(h, opts["total-amount"]), opts


def refused(native, s, needle):
    out = N.LedgerOut()
    st = native.lib().tbc_ledger_check(C.byref(s), C.byref(out))
    msg = native.lib().tbc_last_error().decode()
    assert st == N.ERR_INVALID_ARG, (st, msg)
    assert msg.startswith("tbc_ledger_check") and needle in msg, msg
    return msg


def test_every_invalid_arg_rule_with_its_message(native):
    cols, opts = valid_columns()
    lib = native.lib()
    assert lib.tbc_ledger_check(None, None) == N.ERR_INVALID_ARG and "null argument" in lib.tbc_last_error().decode()
    s, keep = L.ledger_in(cols, opts["accounts"])
    assert lib.tbc_ledger_check(C.byref(s), None) == N.ERR_INVALID_ARG
    for f in ("mop_off", "index", "type", "kind", "flags", "mop_id", "mop_a", "mop_b", "mop_c", "mop_flags", "accounts"):
        s, keep = L.ledger_in(cols, opts["accounts"])
        setattr(s, f, None)
        refused(native, s, "null argument")
    s, keep = L.ledger_in(cols, opts["accounts"])
    s.negative_balances = 2
    refused(native, s, "negative_balances")
    read_row = int(np.flatnonzero((cols.type == 1) & (cols.kind == N.LEDGER_K_READ))[2])

    def broken(field, row, value, needle, op=None):
        s, keep = L.ledger_in(copy.deepcopy(cols), opts["accounts"])          # (the struct points into the columns' own arrays)
        keep[field][row] = value
        msg = refused(native, s, needle)
        if op is not None:
            assert f"op {op} (index {int(keep['index'][op])})" in msg, msg

    broken("mop_off", 0, 1, "mop_off[0] must be 0")
    broken("mop_off", 5, int(cols.mop_off[4]) - 1, "mop_off must be ascending", op=4)
    broken("index", 6, int(cols.index[5]), "strictly ascending", op=6)
    broken("type", 3, 4, "type is not a TBC_LEDGER_T_*", op=3)
    broken("kind", 3, 4, "kind is not a TBC_LEDGER_K_*", op=3)
    broken("flags", 3, 2, "unknown op flags", op=3)
    lo = int(cols.mop_off[read_row])
    broken("mop_flags", lo + 1, 2, "unknown micro-op flags", op=read_row)
    broken("mop_id", lo + 3, int(cols.mop_id[lo]), "names an id twice", op=read_row)
    s, keep = L.ledger_in(copy.deepcopy(cols), opts["accounts"])
    keep["index"][len(cols) - 1] = 0xFFFFFFFF
    refused(native, s, "TBC_NO_OP")
    s, keep = L.ledger_in(cols, [3, 1, 2, 3])
    refused(native, s, "account 3 is listed twice")


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_input_without_a_device_is_no_device(native):
    cols, opts = valid_columns()
    with pytest.raises(N.NoDeviceError):
        L.check_native(cols, opts["accounts"])
    with pytest.raises(N.NoDeviceError):
        L.check_columns([], None)
    t = L.test(opts)                                                           # the composed checker does not fall back either
    h, _ = random_ledger(3, transfers=4, reads=3)
    with pytest.raises(N.NoDeviceError):
        t["checker"].check(t, h)


def test_the_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "ledger_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "planned and checked" in out.stdout and not out.stderr, (out.stdout, out.stderr)
    assert "the launches of 6 shapes" in out.stdout, out.stdout          # (lg::sequence over the recording launcher, against lists written by hand)

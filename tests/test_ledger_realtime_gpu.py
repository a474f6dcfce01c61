"""tbc_ledger_realtime on the MI355X against realtime_numpy of jepsen/ledger.py, exactly: every output array and every summary field
through the C entry point, the result map through realtime_result_map, the composed member through test(realtime=True).  The shape
cases (tests/ledger_realtime_histories.py shape_cases) are the smallest at which a kernel can go wrong: 0 reads, 0 transfers; 1, 8, 65
(more classes than lanes) and 1,025 accounts (past the table in LDS); one account's list of 0, 1, 63, 64, 65 entries and a stream of 62, 64, 66 (a chunk
is 64 entries at these sizes); a transfer of several micro-ops across a chunk edge; every transfer on one account; :ok transfers completed in
the reverse of their invocation order; a read of 300 micro-ops; reads without invocations; sides that name no account; a miss that saturates;
each planted anomaly.  On a valid history every bit is 0, so the bounds arrays are what tells a working kernel from an empty one: they are compared
in every case.  References are computed once."""
import ctypes as C

import numpy as np
import pytest

import ledger_realtime_histories as G
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

pytestmark = pytest.mark.gpu

CASES = G.shape_cases()
PLANTS = [(), ("stale",), ("future",), ("regressed",), G.ANOMALIES]


def assert_same(got, want, tag):
    for k in ("bits", "miss", "lo", "hi", "floor"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")} == want["summary"], tag


def device(history, opts):
    accounts, init, apply_ok = L._rt_opts(None, opts)
    cols = L.LedgerColumns(history)
    return cols, L.check_realtime_native(cols, accounts, init, apply_ok)


@pytest.fixture(scope="module")
def refs(native):
    return {c["name"]: L.realtime_numpy(c["history"], c["opts"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_numpy_statement(refs, case):
    want = refs[case["name"]]
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert want["summary"][k] == v, (case["name"], k)
    cols, got = device(case["history"], case["opts"])
    assert_same(got, want, case["name"])
    gets = ((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ)) | ((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))
    n_gets = int((cols.mop_off[1:][gets] - cols.mop_off[:-1][gets]).sum())   # (the micro-ops copied, if no transfer fails: lookups' are not)
    assert 33 * len(got["lo"]) <= got["summary"]["bytes_in"] <= 33 * n_gets + 64 * 1024 + 24 * len(cols) + 16 * len(case["opts"]["accounts"])
    if want["summary"]["n_checked"]:
        assert (got["hi"] != L._I64_MIN).any()                                # the bounds are there
    for apply_ok in (False,):
        o = dict(case["opts"], **{"ok-transfers-apply?": apply_ok})
        assert_same(device(case["history"], o)[1], L.realtime_numpy(case["history"], o), (case["name"], "ok-transfers-apply? false"))


def test_random_concurrent_ledgers_with_every_planted_anomaly(native):
    for seed, plant in enumerate(PLANTS):
        h, o, planted = G.concurrent_ledger(100 + seed, workers=8, ops=700, plant=plant)
        assert set(planted) == set(plant)
        want = L.realtime_numpy(h, o)
        cols, got = device(h, o)
        assert_same(got, want, plant)
        assert bool(got["summary"]["valid"]) == (not plant)
        for name in plant:                                                     # each plant sets its own bit on the planted read
            r = list(cols.read_ops).index(planted[name])
            assert got["bits"][r] & (3 << (2 * G.ANOMALIES.index(name))), (plant, name)
        accounts, init, apply_ok = L._rt_opts(None, o)
        assert L.realtime_result_map(h, cols, got, accounts, init, apply_ok) == L.RealtimeBounds(o).check(o, h), plant


def test_a_stream_whose_chunks_are_several_wavefronts(native):
    """the reads' stream of more than 4,096 x 64 entries: the plan cuts it into chunks of 128, so every chunk takes a second step of 64
    entries, where a class's carried (count, value) comes from the step before through the chunk's own row"""
    h, o, planted = G.concurrent_ledger(21, workers=16, ops=2600, accounts=64, read_share=0.9, plant=("stale",))
    want = L.realtime_numpy(h, o)
    assert 2 * want["summary"]["n_checked"] > 4096 * 64 and want["summary"]["error_count"] >= 1 and "stale" in planted
    cols, got = device(h, o)
    assert_same(got, want, "chunks of 128 entries")


def test_no_accounts_at_all(native):
    """what only a direct caller of the C entry can ask: every side names no account and is counted, nothing is checked, an amount out
    of range is still found"""
    h, o, _ = G.concurrent_ledger(5, ops=40, fail=0.0)
    cols = L.LedgerColumns(h)
    want = L.realtime_numpy_columns(cols, [], {}, True)
    assert want["summary"]["foreign_sides"] > 0 and want["summary"]["n_checked"] == 0
    assert_same(L.check_realtime_native(cols, [], {}, True), want, "no accounts")
    t = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))[0]
    cols.mop_c[int(cols.mop_off[t])] = 2 ** 31
    with pytest.raises(ValueError, match="outside"):
        L.check_realtime_native(cols, [], {}, True)


def test_composed_member_device_route_equals_host_route(native):
    for plant in ((), G.ANOMALIES):
        h, o, _ = G.concurrent_ledger(7, workers=5, ops=200, plant=plant)
        dev = L.test(o, realtime=True, device_route=True)["checker"].check(o, h)
        host = L.test(o, realtime=True, device_route=False)["checker"].check(o, h)
        assert dev["realtime"] == host["realtime"] and dev["realtime"]["valid?"] == (not plant)
        assert dev == host
    assert "realtime" not in L.test(o)["checker"].check(o, h)


def test_invalid_input_is_refused_with_the_named_message(native):
    h, o, _ = G.concurrent_ledger(3, ops=30)
    accounts, init, apply_ok = L._rt_opts(None, o)

    def refused(change, needle, status=N.ERR_INVALID_ARG):
        s, keep = L.ledger_rt_in(L.LedgerColumns(h), accounts, init, apply_ok)      # (fresh columns: `change` writes into them)
        change(s, keep)
        out = N.LedgerRtOut()
        assert N.lib().tbc_ledger_realtime(C.byref(s), C.byref(out)) == status
        msg = N.lib().tbc_last_error().decode()
        assert msg.startswith("tbc_ledger_realtime") and needle in msg, msg

    refused(lambda s, k: setattr(s, "process", None), "null argument (process)")
    refused(lambda s, k: setattr(s, "ok_transfers_apply", 2), "ok_transfers_apply is 0 or 1")
    refused(lambda s, k: k["init_c"].__setitem__(2, 2 ** 61), "initial value of account 3")
    refused(lambda s, k: k["type"].__setitem__(4, 9), "op 4 (index")
    refused(lambda s, k: k["accounts"].__setitem__(1, 1), "account 1 is listed twice")
    assert N.lib().tbc_ledger_realtime(None, None) == N.ERR_INVALID_ARG


def test_amounts_out_of_range_are_unsupported(native):
    h, o, _ = G.concurrent_ledger(4, ops=40, fail=0.0)
    accounts, init, apply_ok = L._rt_opts(None, o)
    for amount in (-1, 2 ** 31):
        cols = L.LedgerColumns(h)
        t = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))[3]
        cols.mop_c[int(cols.mop_off[t])] = amount
        s, keep = L.ledger_rt_in(cols, accounts, init, apply_ok)
        out = N.LedgerRtOut()
        bits = np.full(len(cols.read_ops), 77, np.uint8)
        out.rt_bits = bits.ctypes.data_as(C.POINTER(C.c_uint8))
        assert N.lib().tbc_ledger_realtime(C.byref(s), C.byref(out)) == N.ERR_UNSUPPORTED
        assert "outside [0, 2^31)" in N.lib().tbc_last_error().decode() and out.summary.bad_amounts == 1
        assert (bits == 77).all()                                              # no results
        with pytest.raises(ValueError, match="outside"):
            L.check_realtime_native(cols, accounts, init, apply_ok)

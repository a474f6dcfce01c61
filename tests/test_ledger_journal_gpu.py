"""tbc_ledger_journal on the MI355X against journal_numpy of jepsen/ledger.py, exactly: every output array and every summary field through
the C entry point, the result map through journal_result_map, the composed member through test(journal=True).  The shape cases
(tests/ledger_journal_histories.py shape_cases) are the smallest at which a kernel can go wrong: 0 lookups, 0 transfers, 0 reads; one
entry; 63 / 64 / 65 and 255 / 256 / 257 entries (a wavefront, a step of the entries kernel's workgroup); 31 / 32 / 33 records (a word of
the bitmap; 63 / 64 / 65 and 255 / 256 / 257 records come with the entries); one record past the LDS window, one past a chunk of the
members kernel and one entry past a slice of a lookup, sized from the plan's constants; 1, 2, 3 and 65 lookups; more reads (8,193), more transfer
micro-ops and chunks of them (524,289) and more slices (2,049 lookups) than the 2,048 workgroups the strided kernels' grids are capped
at, so that each of them takes a second trip on the device; a lookup of only unknown ids; every entry repeated; an id invoked twice with different fields; nil entries and nil records;
foreign sides; transfers ok / fail / info / open; a lookup and a read without invocation; 1, 8, 33 and 1,025 accounts (past the
accounts' table in LDS, and the members kernel's counters past its LDS words); 63 / 64 / 65 reads; partial reads; amounts 0 and 2^31 - 1;
the six plants; a valid concurrent ledger.  Each case has the `counts` it was built for.  n_checked, present and n_entries are positive
where the case has them, so that an empty kernel cannot pass.  The cases are built, and the references computed, once, in a fixture:
collecting this file builds no history."""
import ctypes as C

import numpy as np
import pytest

import ledger_journal_histories as J
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

pytestmark = pytest.mark.gpu

NAMES = J.shape_case_names()
assert_same, bytes_bound = J.assert_same, J.bytes_bound


def device(history, opts):
    accounts, init, apply_ok = L._rt_opts(None, opts)
    cols = L.LedgerColumns(history)
    return cols, L.check_journal_native(cols, accounts, init, apply_ok)


@pytest.fixture(scope="module")
def cases(native):
    return {c["name"]: c for c in J.shape_cases()}


@pytest.fixture(scope="module")
def refs(cases):
    return {name: L.journal_numpy(c["history"], c["opts"]) for name, c in cases.items()}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_numpy_statement(cases, refs, name):
    case, want = cases[name], refs[name]
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        have = want["summary"]["totals"][k] if k in L.JN_KINDS else want["summary"][k]
        assert have > 0 if v == ">0" else have == v, (case["name"], k, have)
    cols, got = device(case["history"], case["opts"])
    assert_same(got, want, case["name"])
    s, E, NL, R, M = (got["summary"],) + L.journal_shapes(cols)
    assert (s["n_entries"], s["n_lookups"], s["read_count"], s["n_xfer_mops"]) == (E, NL, R, M)
    assert s["n_checked"] > 0 or R == 0                                        # an empty kernel cannot pass
    assert got["lk_present"].sum() > 0 or M == 0 or E == 0 or case["name"] == "only-unknown-ids"
    lo, hi = bytes_bound(cols, len(case["opts"]["accounts"]))
    assert lo <= s["bytes_in"] <= hi                                           # 33 bytes a transfer micro-op and an entry, 25 a read micro-op, the head
    assert L.journal_result_map(case["history"], cols, got) == L._jn_map(case["history"], want)


def test_final_lookups_agree_with_lookup_missing(native):
    """the cross-check of the rules: for a :final? lookup, n_records - present is tbc_ledger_check's lookup_missing"""
    for seed, fail in ((21, 0.0), (22, 0.15)):
        h, o, meta = J.journal_ledger(seed, workers=6, ops=300, fail=fail)
        cols, got = device(h, o)
        chk = L.check_native(cols, o["accounts"])
        final = np.array([Lk["final"] for Lk in sorted(meta["lookups"], key=lambda x: x["ret"])], bool).reshape(-1)
        assert final.sum() == len(chk["lookup_missing"]) > 0
        assert np.array_equal(got["summary"]["n_records"] - got["lk_present"][final], chk["lookup_missing"])
        assert (chk["lookup_missing"] > 0).all() == bool(fail)


def test_larger_concurrent_ledgers_plain_and_planted(native):
    for seed, name in enumerate((None,) + J.PLANTS):
        h, o, meta = J.journal_ledger(30 + seed, workers=8, ops=600, fail=0.1 if name == "failed" else 0.0)
        if name is not None:
            h, _ = J.plant(h, meta, name)
        cols, got = device(h, o)
        assert_same(got, L.journal_numpy(h, o), name)
        s = got["summary"]
        assert s["valid"] == (name is None) and s["n_checked"] == 8 * s["read_count"] > 0 and s["n_entries"] > 1000
        kind = {"ahead-of-journal": "ahead"}.get(name, name)
        found = [k for k, v in s["totals"].items() if v]                       # (a journal that lacks or gains a transfer also moves its books: ahead / behind beside it)
        assert kind in found if name else not found


def test_composed_member_device_route_equals_host_route(native):
    hp, o, _counts = J.planted("altered")
    dev = L.test(o, realtime=True, snapshots=True, journal=True, device_route=True)["checker"].check(o, hp)
    host = L.test(o, realtime=True, snapshots=True, journal=True, device_route=False)["checker"].check(o, hp)
    assert dev == host
    assert dev["journal"]["valid?"] is False and dev["valid?"] is False and list(dev["journal"]["errors"]) == ["altered"]
    assert all(dev[k]["valid?"] is True for k in J.MEMBERS)                    # the flipped bit passes every other member
    h, o, _ = J.journal_ledger(7, workers=5, ops=200)
    res = L.test(o, journal=True)["checker"].check(o, h)["journal"]
    assert res == L.JournalAudit(o).check(o, h) and res["valid?"] is True and res["entry-count"] > 0
    assert "journal" not in L.test(o)["checker"].check(o, h)


def test_ok_transfers_apply_false_reports_nothing_lost(native):
    hp, o, counts = J.planted("lost")
    accounts, init, _ = L._rt_opts(None, o)
    cols = L.LedgerColumns(hp)
    got = L.check_journal_native(cols, accounts, init, False)
    assert_same(got, L.journal_numpy_columns(cols, accounts, init, False), "apply false")
    assert got["summary"]["totals"]["lost"] == 0 and got["summary"]["valid"] == 1


def test_invalid_input_is_refused_with_the_named_message(native):
    h, o, _ = J.journal_ledger(3, ops=40)
    accounts, init, apply_ok = L._rt_opts(None, o)

    def refused(change, needle):
        s, keep = L.ledger_rt_in(L.LedgerColumns(h), accounts, init, apply_ok)     # (fresh columns: `change` writes into them)
        change(s, keep)
        out = N.LedgerJournalOut()
        assert N.lib().tbc_ledger_journal(C.byref(s), C.byref(out)) == N.ERR_INVALID_ARG
        msg = N.lib().tbc_last_error().decode()
        assert msg.startswith("tbc_ledger_journal") and needle in msg, msg

    refused(lambda s, k: setattr(s.ledger, "mop_off", None), "null argument (mop_off)")
    refused(lambda s, k: setattr(s, "process", None), "null argument (process)")
    refused(lambda s, k: k["type"].__setitem__(4, 9), "op 4 (index")
    refused(lambda s, k: k["accounts"].__setitem__(1, 1), "account 1 is listed twice")
    refused(lambda s, k: k["index"].__setitem__(5, int(k["index"][4])), "strictly ascending")
    refused(lambda s, k: k["init_c"].__setitem__(2, 2 ** 61), "2^61")
    refused(lambda s, k: setattr(s, "ok_transfers_apply", 2), "ok_transfers_apply")
    assert N.lib().tbc_ledger_journal(None, None) == N.ERR_INVALID_ARG


def test_an_amount_out_of_range_is_unsupported_and_leaves_the_arrays_alone(cases):
    case = cases["65-entries"]
    accounts, init, apply_ok = L._rt_opts(None, case["opts"])
    for amount in (2 ** 31, -1):
        cols = L.LedgerColumns(case["history"])
        tr = np.flatnonzero((cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER))
        cols.mop_c[int(cols.mop_off[tr[40]])] = amount
        s, keep = L.ledger_rt_in(cols, accounts, init, apply_ok)
        out, arr, _ = L.journal_out(cols, len(accounts))
        for x in arr.values():
            x[:] = 77
        assert N.lib().tbc_ledger_journal(C.byref(s), C.byref(out)) == N.ERR_UNSUPPORTED
        assert "2^31" in N.lib().tbc_last_error().decode() and out.summary.bad_amounts == 1
        assert all((x == 77).all() for x in arr.values())                      # no results
        with pytest.raises(ValueError, match="2\\^31"):
            L.check_journal_native(cols, accounts, init, apply_ok)

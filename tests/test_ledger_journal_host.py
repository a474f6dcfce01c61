"""The journal audit on the CPU (jepsen/ledger.py, "Journal audit"): journal_host, the specification, against answers derived by hand
for every rule; journal_numpy, the statement the device is compared with, against journal_host on the shape cases and on seeded random
histories, damaged and not; the cross-check of the rules against lookup-transfers; which of the existing members still pass each plant;
every ValueError; the checker and the composed member on the host route."""
import random

import numpy as np
import pytest

import ledger_journal_histories as J
from conftest import has_gpu
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

NO = N.NO_OP
A3 = [1, 2, 3]


def totals(res):
    return {k: v for k, v in res["summary"]["totals"].items() if v}


def same(a, b, tag):
    for k in L.JN_ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (tag, k)
    assert a["summary"] == b["summary"], tag


def test_entries_unknown_altered_repeated_by_hand():
    # records: id 1 (1 -> 2, 5), id 2 nil, id 3 (2 -> 3, 7); id 1 is invoked again with other fields: reinvoked, no record
    transfers = [[(1, 1, 2, 5)], [(2, None, None, None)], [(3, 2, 3, 7)], [(1, 3, 3, 9)]]
    lookup = [(1, 1, 2, 5), (1, 1, 2, 5), (9, 1, 2, 5), (2, None, None, None), (3, 2, 3, 8), (3, None, None, None), (1, 3, 3, 9)]
    h, o = J.staged(A3, transfers, [lookup], reads=0)
    res = L.journal_host(h, o)
    #        same  same  unknown  both nil  amount  nil entry  the reinvoked micro-op's fields, not the record's
    assert res["entry_bits"].tolist() == [0, 0, 1, 2, 2, 2, 2]
    assert res["xfer_flags"].tolist() == [0, 2, 0, 1]
    assert res["lk_present"].tolist() == [3]
    assert res["lk_counts"][0].tolist() == [1, 4, 3, 0, 0, 0, 0, 0, 0]          # repeated: 6 entries with a record - 3 present
    # the books move by the RECORDS present that are not nil, whatever the entries say: 5 from 1 to 2, 7 from 2 to 3
    assert res["lk_vector"][0].tolist() == [0, 5, 5, 7, 7, 0]
    s = res["summary"]
    assert (s["n_records"], s["n_reinvoked"], s["n_xfer_mops"], s["n_entries"], s["n_lookups"], s["foreign_sides"]) == (3, 1, 4, 7, 1, 2)
    assert s["valid"] == 0 and s["errors"]["altered"] == {"count": 1, "first": 0, "last": 0, "worst": 0} and s["errors"]["failed"]["first"] == NO
    assert res["xfer_present"].tolist() == [1, 1, 1, 0]
    same(L.journal_numpy(h, o), res, "by hand")


def test_failed_early_lost_vanished_by_hand():
    # history positions: t1 0-1 ok, t2 2-3 fail, t3 4-5 info, t4 6 open, lookups 7-8, 9-10, 11-12, then t5 13-14 ok
    transfers = [[(1, 1, 2, 1)], [(2, 1, 2, 2)], [(3, 1, 2, 3)], [(4, 1, 2, 4)]]
    first, second, third = [(1, 1, 2, 1), (2, 1, 2, 2), (3, 1, 2, 3), (5, 2, 3, 6)], [(3, 1, 2, 3)], [(4, 1, 2, 4)]
    h, o = J.staged(A3, transfers, [first, second, third], reads=0, statuses=["ok", "fail", "info", "open"])
    J._op(h, 50, "invoke", [J._t(5, 2, 3, 6)])
    J._op(h, 50, "ok", [J._t(5, 2, 3, 6)])
    res = L.journal_host(h, o)
    # lookup 0 shows 1, 2 (failed), 3 and 5, which is invoked after it completed (early); 4 is open: absent, not lost
    # lookup 1 shows 3: 1 is ok before it began -> lost, and shown before -> vanished; 2 vanished; 5 vanished; 4 never shown
    # lookup 2 shows 4: 1 lost + vanished, 2 vanished, 3 vanished (info: not lost), 5 vanished
    assert res["lk_counts"][:, 3:7].tolist() == [[1, 1, 0, 0], [0, 0, 1, 3], [0, 0, 1, 4]]
    assert res["lk_present"].tolist() == [4, 1, 1]
    assert (res["xfer_present"].tolist(), res["xfer_early"].tolist()) == ([1, 1, 2, 1, 1], [0, 0, 0, 0, 1])
    assert (res["xfer_lost"].tolist(), res["xfer_vanished"].tolist()) == ([2, 0, 0, 0, 0], [2, 2, 1, 0, 2])
    s = res["summary"]
    assert s["errors"]["vanished"] == {"count": 2, "first": 1, "last": 2, "worst": 2} and s["errors"]["lost"] == {"count": 2, "first": 1, "last": 2, "worst": 1}
    assert s["totals"]["vanished"] == 7 and s["totals"]["failed"] == 1
    same(L.journal_numpy(h, o), res, "by hand")
    # ok-transfers-apply? false: nothing is lost; a lookup without invocation has nothing before it
    off = L.journal_host(h, dict(o, **{"ok-transfers-apply?": False}))
    assert off["summary"]["totals"]["lost"] == 0 and off["summary"]["totals"]["vanished"] == 7
    hb, ob = J.staged(A3, transfers, [second, first, third], reads=0, statuses=["ok", "fail", "info", "open"], bare=True)
    bare = L.journal_host(hb, ob)
    assert bare["lk_counts"][0, 3:7].tolist() == [0, 0, 0, 0] and bare["lk_counts"][1, 5:7].tolist() == [0, 0]
    m = L._jn_map(h, res)
    assert m["errors"]["failed"]["ids"] == [2] and m["errors"]["early"]["ids"] == [5] and m["errors"]["lost"]["ids"] == [1] and m["errors"]["vanished"]["ids"] == [1, 2, 3, 5]
    assert m["errors"]["vanished"]["worst"] is h[12] and m["errors"]["failed"]["first"] is h[8] and m["errors"]["lost"]["total"] == 2


def test_books_and_reads_by_hand():
    init = {1: {"credits-posted": 10, "debits-posted": 1}}
    # t1 (1 -> 2, 5) ok; t2 (3 -> 99, 7), a foreign credit side; reads: before the transfers, after them, after the lookups
    h, o = J.staged(A3, [[(1, 1, 2, 5)], [(2, 3, 99, 7)]], [[(1, 1, 2, 5)], [(1, 1, 2, 5), (2, 3, 99, 7)]], reads=3, init=init)
    res = L.journal_host(h, o)
    #                                          c1  d1 c2 d2 c3 d3
    assert res["lk_vector"].tolist() == [[10, 6, 5, 0, 0, 0], [10, 6, 5, 0, 0, 7]]
    assert res["summary"]["foreign_sides"] == 1 and res["summary"]["n_checked"] == 9
    # read 1 (after both transfers) shows debits of 7 on account 3 and completed before lookup 0 began, whose books lack transfer 2: ahead
    assert res["rd_bits"].tolist() == [0, 1, 0] and res["rd_first"].tolist() == [[NO, NO], [0, NO], [NO, NO]]
    assert res["lk_counts"][:, 7:].tolist() == [[1, 0], [0, 0]]
    # the last read comes back without transfer 1: behind both lookups, which completed before it began
    h2 = [dict(op) for op in h]
    h2[-1] = dict(h2[-1], value=[["r", 1, {"credits-posted": 10, "debits-posted": 1}], ["r", 2, {"credits-posted": 5, "debits-posted": 0}],
                                 ["r", 3, {"credits-posted": 0, "debits-posted": 7}]])
    res2 = L.journal_host(h2, o)
    assert res2["rd_bits"].tolist() == [0, 1, 2] and res2["rd_first"][2].tolist() == [NO, 0] and res2["lk_counts"][:, 8].tolist() == [1, 1]
    same(L.journal_numpy(h2, o), res2, "by hand")
    # a counter the read does not check is not compared: the same read, account 1 left out
    h3 = h2[:-1] + [dict(h2[-1], value=h2[-1]["value"][1:])]
    assert L.journal_host(h3, o)["rd_bits"].tolist() == [0, 1, 0] and L.journal_host(h3, o)["summary"]["n_checked"] == 8


CASES = J.shape_cases(big=False)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_numpy_statement_equals_the_specification(case):
    want = L.journal_host(case["history"], case["opts"])
    same(L.journal_numpy(case["history"], case["opts"]), want, case["name"])
    for k, v in case["counts"].items():
        have = want["summary"]["totals"][k] if k in L.JN_KINDS else want["summary"][k]
        assert have > 0 if v == ">0" else have == v, (case["name"], k, have)


def test_numpy_statement_equals_the_specification_on_random_histories():
    rng = random.Random(11)
    for seed in range(8):
        h, o, meta = J.journal_ledger(seed, workers=2 + seed % 4, ops=60, fail=0.1 * (seed % 3), accounts=1 + seed)
        if seed >= 3:                                                          # damage: entries dropped, doubled, changed, made up, nil
            for Lk in meta["lookups"]:
                v = h[Lk["ret"]]["value"] = [list(m[:2]) + [dict(m[2])] for m in h[Lk["ret"]]["value"]]
                for _ in range(rng.randint(0, 3)):
                    k, how = rng.randrange(len(v)), rng.randrange(5)
                    if how == 0 and len(v) > 1: del v[k]
                    elif how == 1: v.append(v[k])
                    elif how == 2: v[k][2]["amount"] += 1
                    elif how == 3: v.append(["l-t", 10 ** 6 + k, dict(v[k][2])])
                    else: v[k][2] = None
        same(L.journal_numpy(h, o), L.journal_host(h, o), seed)
        if seed < 3:
            assert L.journal_host(h, o)["summary"]["valid"] == 1               # valid by construction, failed transfers or not


def test_final_lookups_agree_with_lookup_all_invoked_transfers():
    """n_records - present[L] of a :final? lookup is lookup_missing: lookup-transfers suspects exactly the final lookups where it is not 0"""
    for seed, fail in ((4, 0.0), (5, 0.2), (6, 0.2)):
        h, o, meta = J.journal_ledger(seed, workers=4, ops=80, fail=fail)
        if seed == 6:
            h[meta["lookups"][-1]["ret"]] = dict(h[meta["lookups"][-1]["ret"]], value=h[meta["lookups"][-1]["ret"]]["value"] + [["l-t", t["mops"][0][1], t["mops"][0][2]] for t in meta["transfers"] if t["status"] == "fail" for _ in (0,)])
        res = L.journal_host(h, o)
        lookups = sorted(meta["lookups"], key=lambda x: x["ret"])
        missing = res["summary"]["n_records"] - res["lk_present"].astype(np.int64)
        suspect = L.LookupAllInvokedTransfers().check(o, h).get("suspect-final-lookups", [])
        assert [h[Lk["ret"]] for k, Lk in enumerate(lookups) if Lk["final"] and missing[k]] == suspect
        invoked = {m[1] for op in h if op["type"] == "invoke" and L.op_txn_f(op) == "t" for m in op["value"]}
        for k, Lk in enumerate(lookups):
            assert missing[k] == len(invoked - {m[1] for m in h[Lk["ret"]]["value"]})
        assert bool(suspect) == bool(fail)


@pytest.mark.parametrize("name", J.PLANTS)
def test_each_plant_is_found_and_passes_the_members_it_is_said_to_pass(name):
    hp, o, counts = J.planted(name)
    res = L.test(o, realtime=True, snapshots=True, journal=True, device_route=False)["checker"].check(o, hp)
    assert tuple(k for k in J.MEMBERS if res[k]["valid?"] is True) == J.PASSES[name]
    assert res["journal"]["valid?"] is False and res["valid?"] is False
    kind = {"ahead-of-journal": "ahead"}.get(name, name)
    assert list(res["journal"]["errors"]) == [kind]
    want = counts[kind]
    assert res["journal"]["errors"][kind]["total"] > 0 if want == ">0" else res["journal"]["errors"][kind]["total"] == want
    assert J.PASSES["altered"] == J.MEMBERS and J.PASSES["ahead-of-journal"] == J.MEMBERS      # a flipped amount and money ahead of the journal pass all five


def test_the_member_is_composed_only_when_asked_for():
    h, o, _ = J.journal_ledger(2, ops=50)
    plain = L.test(o, device_route=False)["checker"].check(o, h)
    with_journal = L.test(o, journal=True, device_route=False)["checker"].check(o, h)
    assert "journal" not in plain and {k: v for k, v in with_journal.items() if k != "journal"} == plain
    assert with_journal["journal"] == L.JournalAudit(o).check(o, h) == {"valid?": True, "lookup-count": with_journal["journal"]["lookup-count"],
                                                                        "entry-count": with_journal["journal"]["entry-count"], "record-count": with_journal["journal"]["record-count"],
                                                                        "reinvoked-count": 0, "errors": {}}
    assert with_journal["journal"]["entry-count"] > 0


def test_every_value_error():
    h, o = J.staged(A3, [[(1, 1, 2, 5)], [(2, 2, 3, 2 ** 31)]], [[(1, 1, 2, 5)]])
    for f in (L.journal_host, L.journal_numpy):
        with pytest.raises(ValueError, match="not in \\[0, 2\\^31\\)"):
            f(h, o)
    h, o = J.staged(A3, [[(1, 1, 2, -1)]], [[(1, 1, 2, 5)]])
    for f in (L.journal_host, L.journal_numpy):
        with pytest.raises(ValueError, match="not in \\[0, 2\\^31\\)"):
            f(h, o)
    # the amount of a micro-op that is no record is nobody's: a reinvoked id, and an entry's own amount
    h, o = J.staged(A3, [[(1, 1, 2, 5)], [(1, 1, 2, 2 ** 40)]], [[(1, 1, 2, 2 ** 40)]])
    assert L.journal_host(h, o)["summary"]["totals"]["altered"] == 1 == L.journal_numpy(h, o)["summary"]["totals"]["altered"]
    h, o = J.staged(A3, [[(1, 1, 2, 5)]], [[(1, 1, 2, 5)]], init={1: {"credits-posted": 2 ** 61, "debits-posted": 0}})
    for f in (L.journal_host, L.journal_numpy):
        with pytest.raises(ValueError, match="2\\^61"):
            f(h, o)
    with pytest.raises(ValueError, match="2\\^31 or more transfer micro-ops"):
        L._jn_ranges([], 2 ** 31, [], {})
    with pytest.raises(ValueError, match="a lookup of 2\\^31 or more entries"):
        L._jn_ranges([], 0, [5, 2 ** 31], {})


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_input_without_a_device_is_no_device(native):
    h, o, _ = J.journal_ledger(2, ops=50)
    accounts, init, apply_ok = L._rt_opts(None, o)
    with pytest.raises(N.NoDeviceError):
        L.check_journal_native(L.LedgerColumns(h), accounts, init, apply_ok)
    t = L.test(o, journal=True)                                                # the composed member does not fall back either
    with pytest.raises(N.NoDeviceError):
        t["checker"].check(t, h)

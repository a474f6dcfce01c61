"""The host statement of the ledger workload's checkers (jepsen/ledger.py: ledger_to_bank, BankChecker, UnexpectedOps,
LookupAllInvokedTransfers, FinalReads -- the reference's tests/ledger.clj:89-282) on hand-derived histories with the expected maps
written out, and on the hand-made EDN histories of tests/golden/ledger/ (their expectations are derived in its README.md)."""
import os

from conftest import ROOT
from jepsen_tigerbeetle_amd.jepsen import edn
from jepsen_tigerbeetle_amd.jepsen import ledger as L
from ledger_histories import Builder, r_mop, t_mop

GOLDEN = os.path.join(ROOT, "tests", "golden", "ledger")
OPTS3 = {"accounts": [1, 2, 3], "total-amount": 0, "negative-balances?": False}


def golden(name):
    return edn.read_history(os.path.join(GOLDEN, name))


def test_ledger_to_bank_maps_each_kind_of_op():
    b = Builder()
    b.transfer(7, 1, 2, 5)
    b.read([r_mop(1, 10, 4), r_mop(2, 3, 0)], process=1)
    b.nemesis()
    b.read([r_mop(1, 1, 0)], process=2, complete="info")
    b.lookup([(7, 1, 2, 5)], process=1, final=True)
    bank = L.ledger_to_bank(b.h)
    h = b.h
    assert bank == [
        dict(h[0], f="transfer"), dict(h[1], f="transfer"),
        dict(h[2], f="read"), dict(h[3], f="read", value={1: 6, 2: 3}),
        h[4],                                                               # (no integer :process: kept as it is)
        dict(h[5], f="read"), dict(h[6], f="read"),                         # (:info :r keeps its value)
    ]                                                                       # (:l-t ops are dropped, whatever their type)
    assert bank[4] is h[4] and bank[0]["value"] == [t_mop("t", 7, 1, 2, 5)]


def test_ledger_to_bank_last_micro_op_of_an_id_wins_and_empty_values_are_skipped():
    b = Builder()
    b.read([r_mop(1, 99, 0), r_mop(2, 5, 0), r_mop(1, 7, 2)])
    b.op("invoke", [], 3)
    b.op("ok", None, 3)
    bank = L.ledger_to_bank(b.h)
    assert [o["index"] for o in bank] == [0, 1] and bank[1]["value"] == {1: 5, 2: 5}
    res = L.BankChecker({"negative-balances?": False}).check({"accounts": [1, 2], "total-amount": 10}, b.h)
    assert res == {"valid?": True, "read-count": 1, "error-count": 0, "first-error": None, "errors": {}}
    # no checker counts the ops without a first micro-op
    assert L.FinalReads().check(None, b.h) == {"valid?": False, "unequal-final-reads": [], "unequal-final-lookups": []}
    assert L.LookupAllInvokedTransfers().check(None, b.h) == {"valid?": True}


def test_cond_priority_and_each_error_map():
    test = {"accounts": [1, 2], "total-amount": 10}
    b = Builder()
    b.read([r_mop(1, 0, 5), r_mop(2, 16, 0)])                  # -5 + 16 = 11: wrong total AND negative -> wrong-total
    b.read([r_mop(1, 0, 5), r_mop(2, 15, 0)])                  # total 10, negative
    b.read([r_mop(1, 10, 0), r_mop(3, 1, 0)])                  # unexpected key AND wrong total -> unexpected-key
    b.read([["r", 1, None], r_mop(5, 1, 0)])                   # unexpected key AND nil -> unexpected-key
    b.read([["r", 1, None], r_mop(2, 1, 0)])                   # nil AND wrong total -> nil-balance
    res = L.BankChecker({"negative-balances?": False}).check(test, b.h)
    bank = L.ledger_to_bank(b.h)
    wt = {"type": "wrong-total", "total": 11, "op": bank[1]}
    nv = {"type": "negative-value", "negative": [-5], "op": bank[3]}
    uk1 = {"type": "unexpected-key", "unexpected": [3], "op": bank[5]}
    uk2 = {"type": "unexpected-key", "unexpected": [5], "op": bank[7]}
    nb = {"type": "nil-balance", "nils": {1: None}, "op": bank[9]}
    assert res == {"valid?": False, "read-count": 5, "error-count": 5, "first-error": wt,
                   "errors": {"wrong-total": {"count": 1, "first": wt, "worst": wt, "last": wt, "lowest": wt, "highest": wt},
                              "negative-value": {"count": 1, "first": nv, "worst": nv, "last": nv},
                              "unexpected-key": {"count": 2, "first": uk1, "worst": uk1, "last": uk2},
                              "nil-balance": {"count": 1, "first": nb, "worst": nb, "last": nb}}}
    # with negative balances allowed the second read is fine, the first still a wrong total
    res = L.BankChecker({"negative-balances?": True}).check(test, b.h)
    assert res["error-count"] == 4 and "negative-value" not in res["errors"] and res["errors"]["wrong-total"]["count"] == 1


def test_worst_lowest_highest_ties_go_to_the_earliest():
    test = {"accounts": [1, 2], "total-amount": 10}
    b = Builder()
    for total in (12, 8, 13, 7, 13, 7, 10):                    # distances 2 2 3 3 3 3 0
        b.read([r_mop(1, total - 1, 0), r_mop(2, 1, 0)])
    e = L.BankChecker().check(test, b.h)["errors"]["wrong-total"]
    assert e["count"] == 6 and e["first"]["op"]["index"] == 1 and e["last"]["op"]["index"] == 11
    assert e["worst"]["op"]["index"] == 5                      # |13 - 10| = |7 - 10| = 3: the first of the four
    assert e["highest"]["op"]["index"] == 5 and e["highest"]["total"] == 13
    assert e["lowest"]["op"]["index"] == 7 and e["lowest"]["total"] == 7
    # negative-value: badness is minus the sum of the negatives; unexpected-key: how many
    b = Builder()
    b.read([r_mop(1, 0, 3), r_mop(2, 13, 0)])
    b.read([r_mop(1, 0, 5), r_mop(2, 15, 0)])
    b.read([r_mop(1, 0, 5), r_mop(2, 15, 0)])
    e = L.BankChecker().check(test, b.h)["errors"]["negative-value"]
    assert (e["worst"]["op"]["index"], e["first"]["op"]["index"], e["last"]["op"]["index"]) == (3, 1, 5)


def test_unexpected_ops_with_an_open_invoke_and_a_fail():
    b = Builder()
    b.transfer(1, process=0)
    b.transfer(2, process=1, complete=None)                    # index 2, time 3000: open
    b.read([r_mop(1, 0, 0)], process=2, complete="fail")       # index 3, 4
    b.transfer(3, process=0, complete="info")                  # index 5, 6 (time 7000): an :info completes its invoke
    b.nemesis()
    res = L.UnexpectedOps().check(None, b.h)
    assert res == {"valid?": "unknown", "open-ops": [((7000 - 3000) / 1e6, b.h[2])], "fail-ops": [b.h[4]]}
    b = Builder()
    b.transfer(1)
    assert L.UnexpectedOps().check(None, b.h) == {"valid?": True}


def test_lookup_all_invoked_transfers():
    b = Builder()
    b.transfer(1); b.transfer(2, complete="fail"); b.transfer(3, complete=None, process=4)
    b.op("ok", [t_mop("t", 9, 1, 2, 1)], 3)                    # (an :ok transfer nobody invoked is not an invoked transfer)
    b.lookup([(1, 1, 2, 1), (2, 1, 2, 1), (3, 1, 2, 1)], process=0)
    b.lookup([(3, 1, 2, 1), (1, 1, 2, 1), (1, 1, 2, 1), (77, 1, 2, 1)], process=1)       # 2 is missing; repeats and strangers do not help
    b.lookup([(1, 1, 2, 1)], process=2, final=False)           # not final: not looked at
    b.lookup([], process=3, complete="info")
    res = L.LookupAllInvokedTransfers().check(None, b.h)
    suspect = [o for o in b.h if o["type"] == "ok" and o["process"] == 1 and o.get("final?")]
    assert len(suspect) == 1 and res == {"valid?": False, "suspect-final-lookups": suspect}


def test_final_reads():
    row = [r_mop(1, 5, 0), r_mop(2, 5, 0)]
    b = Builder()
    b.transfer(1)
    b.read(row, 0, final=True); b.read(row, 1, final=True)
    b.lookup([(1, 1, 2, 1)], 0); b.lookup([(1, 1, 2, 1)], 1)
    assert L.FinalReads().check(None, b.h) == {"valid?": True}
    b.read(row[::-1], 2, final=True)                           # the same micro-ops in another order: another vector
    assert L.FinalReads().check(None, b.h) == {"valid?": False, "unequal-final-reads": [row, row[::-1]]}
    b = Builder()
    b.read(row, 0, final=True)                                 # final reads but no final lookup at all
    assert L.FinalReads().check(None, b.h) == {"valid?": False, "unequal-final-lookups": []}


def test_the_composed_test_map_and_its_defaults():
    t = L.test(device_route=False)
    assert (t["accounts"], t["max-transfer"], t["total-amount"], t["negative-balances?"]) == (list(range(1, 9)), 5, 0, False)
    assert sorted(t["checker"].checkers) == ["SI", "final-reads", "lookup-transfers", "unexpected-ops"]
    assert sorted(L.test(linear=True)["checker"].checkers) == ["SI", "final-reads", "linear", "lookup-transfers", "unexpected-ops"]
    t = L.test({"accounts": [4, 5], "total-amount": 7, "negative-balances?": True}, device_route=False)
    assert (t["accounts"], t["max-transfer"], t["total-amount"]) == ([4, 5], 5, 7)


def test_golden_valid_history():
    h = golden("valid.edn")
    assert len(h) == 13 and h[4]["process"] == "nemesis" and h[5]["final?"] is True
    t = L.test(dict(OPTS3, **{"negative-balances?": True}), device_route=False)
    res = t["checker"].check(t, h)
    assert res == {"valid?": True, "SI": {"valid?": True, "read-count": 3, "error-count": 0, "first-error": None, "errors": {}},
                   "lookup-transfers": {"valid?": True}, "final-reads": {"valid?": True}, "unexpected-ops": {"valid?": True}}
    t = L.test(OPTS3, device_route=False)
    e = t["checker"].check(t, h)["SI"]["errors"]
    assert list(e) == ["negative-value"] and e["negative-value"]["count"] == 3
    assert [e["negative-value"][f]["op"]["index"] for f in ("first", "worst", "last")] == [3, 3, 8]


def test_golden_history_with_every_anomaly():
    h = golden("anomalies.edn")
    t = L.test(OPTS3, device_route=False)
    res = t["checker"].check(t, h)
    assert res["valid?"] is False
    si = res["SI"]
    assert (si["valid?"], si["read-count"], si["error-count"], si["first-error"]["op"]["index"]) == (False, 7, 7, 5)
    at = lambda t_, f: si["errors"][t_][f]["op"]["index"]
    assert {t_: e["count"] for t_, e in si["errors"].items()} == {"negative-value": 3, "wrong-total": 2, "unexpected-key": 1, "nil-balance": 1}
    assert [at("negative-value", f) for f in ("first", "worst", "last")] == [5, 5, 20]
    assert [at("wrong-total", f) for f in ("first", "worst", "last", "lowest", "highest")] == [7, 7, 9, 9, 7]
    assert si["errors"]["wrong-total"]["lowest"]["total"] == -2 and si["errors"]["wrong-total"]["highest"]["total"] == 2
    assert si["errors"]["unexpected-key"]["first"]["unexpected"] == [9] and at("unexpected-key", "first") == 11
    assert si["errors"]["nil-balance"]["first"]["nils"] == {1: None} and at("nil-balance", "first") == 13
    assert si["errors"]["negative-value"]["first"]["negative"] == [-3]
    assert si["errors"]["negative-value"]["first"]["op"]["value"] == {1: -3, 2: 3, 3: 0}
    assert res["lookup-transfers"] == {"valid?": False, "suspect-final-lookups": [h[22]]}
    assert res["final-reads"] == {"valid?": False, "unequal-final-reads": [h[18]["value"], h[20]["value"]],
                                  "unequal-final-lookups": [h[22]["value"], h[24]["value"]]}
    assert res["unexpected-ops"] == {"valid?": "unknown", "open-ops": [(8.0, h[16])], "fail-ops": [h[15]]}

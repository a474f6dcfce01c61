"""tbc_ledger_check on the MI355X against the host statement of jepsen/ledger.py, exactly: the raw arrays and the summary through the C
entry point, the three result maps through check_columns.  The shapes (tests/ledger_histories.py shape_cases) are the smallest at which
each kernel can go wrong:
  reads          exactly 0, 1, 63 / 64 / 65, 255 / 256 / 257, 513 :ok reads (of 8 micro-ops: 32 reads a run; of 1: 256 reads a run)
  micro-ops      1, 8, 63-65 a read, one read of 300 among short ones (a run of its own, taken in steps), sizes that straddle runs
  accounts       1, 8, 70 and 1,100 (more than the kernel keeps in LDS), handed over unsorted
  totals         near +-2^62 with total-amount far from 0; credits and debits near 2^58; negative-balances? both ways, every case
  transfers |T|  0, 1, 31 / 32 / 33, 255-257; once 32 x 8,192 + 1, which takes a second window
  final lookups  0, 1, 2, 70; with repeated ids and with ids nobody invoked; with transfers missing (the first, the last, a middle one)
  final rows     that differ from the first in the last micro-op only, one field only, the NIL flag only, order only, length only; none
Every reference is computed once (module fixture), which first asserts that the inputs are not vacuous and that each case has the
shape it is named for (ledger_histories.references)."""
import os

import numpy as np
import pytest

import ledger_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import edn
from jepsen_tigerbeetle_amd.jepsen import ledger as L

pytestmark = pytest.mark.gpu

CASES = G.shape_cases()


@pytest.fixture(scope="module")
def refs(native):
    return G.references(CASES)


def host_maps(h, o):
    return {"SI": L.BankChecker(o).check(o, h), "lookup-transfers": L.LookupAllInvokedTransfers().check(o, h), "final-reads": L.FinalReads().check(o, h)}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_host_statement(refs, case):
    name = case["name"]
    for neg in (False, True):
        h, o, want = refs[(name, neg)]
        cols = L.LedgerColumns(h, o["total-amount"])
        if "ok_reads" in case:
            assert len(cols.read_ops) == case["ok_reads"]                     # the device gets the number of :ok reads the case is named for
        got = L.check_native(cols, o["accounts"], neg)
        G.assert_same(got, want, (name, neg))
        assert got["summary"]["bytes_in"] >= 33 * len(cols.mop_id)
        assert L.check_columns(h, o) == host_maps(h, o), (name, neg)


def test_random_ledgers_with_every_planted_anomaly(native):
    plants = [(), ("wrong-total", "negative"), ("unexpected", "nil", "dup-id"), ("missing-transfer",), ("final-read-field", "final-lookup-order"),
              ("final-read-order", "final-lookup-field"), ("final-lookup-length", "final-read-length"), ("no-final",),
              ("wrong-total", "negative", "unexpected", "nil", "dup-id", "final-read-length", "final-lookup-field")]
    inputs = [G.random_ledger(seed, workers=7, transfers=400, reads=300, info=0.04 * (seed % 2), fail=0.03 * (seed % 2), plant=p)
              for seed, p in enumerate(plants)]
    wants = [G.expected(h, o) for h, o in inputs]
    for (h, o), want, p in zip(inputs, wants, plants):                        # every plant has landed, and the plain input is fully valid
        assert set(p or ("valid",)) <= G.landed(h, want["summary"]), (p, G.landed(h, want["summary"]))
    assert set().union(*plants) == set(G.ANOMALIES)
    for (h, o), want, p in zip(inputs, wants, plants):
        G.assert_same(L.check_native(L.LedgerColumns(h, o["total-amount"]), o["accounts"], False), want, p)
        assert L.check_columns(h, o) == host_maps(h, o), p


def test_more_transfers_than_one_window_holds(native):
    """|T| = 32 x 8,192 + 1 and two final lookups: one complete, the other without one id of the first window and without the last id,
    which lives in the second."""
    T = 32 * N.LEDGER_LOOKUP_WINDOW_WORDS + 1
    b = G.Builder()
    for i in range(T):
        b.op("invoke", [G.t_mop("t", 7 * i + 1, 1, 2, 1)], i % 64)
    full = [G.t_mop("l-t", 7 * i + 1, 1, 2, 1) for i in range(T)]
    b.op("ok", full, 0, final=True)
    b.op("ok", full[:1234] + full[1235:T - 1], 1, final=True)
    cols = L.LedgerColumns(b.h)
    got = L.check_native(cols, [1, 2])
    s = got["summary"]
    assert s["n_transfers"] == T and got["lookup_missing"].tolist() == [0, 2]
    assert (s["suspect_lookups"], s["valid_lookups"], s["n_final_lookups"], s["final_lookups_unlike"]) == (1, 0, 2, 1)
    assert got["final_lookup_unlike"].tolist() == [0, 1]
    assert (s["valid_final_reads"], s["n_final_reads"], s["read_count"], s["valid_si"]) == (0, 0, 0, 1)
    # the host statement says the same of the suspect lookup
    assert L.LookupAllInvokedTransfers().check(None, b.h) == {"valid?": False, "suspect-final-lookups": [b.h[-1]]}


def test_the_composed_checker_with_the_linear_member_on_a_golden_history(native):
    h = edn.read_history(os.path.join(ROOT, "tests", "golden", "ledger", "valid.edn"))
    opts = {"accounts": [1, 2, 3], "total-amount": 0, "negative-balances?": True}
    dev, host = L.test(opts, linear=True, device_route=True), L.test(opts, linear=True, device_route=False)
    got, want = dev["checker"].check(dev, h), host["checker"].check(host, h)
    untimed = lambda a: {k: v for k, v in a.items() if k != "stats"}               # (a search's stats hold its times)
    got["linear"], want["linear"] = untimed(got["linear"]), untimed(want["linear"])
    assert sorted(got) == ["SI", "final-reads", "linear", "lookup-transfers", "unexpected-ops", "valid?"]
    shared = dev["checker"].checkers["SI"].shared                                  # one device call served the three members, and is let go
    assert shared.key is None and shared.res is None and dev["checker"].checkers["final-reads"].shared is shared
    assert got == want and got["valid?"] is True and got["linear"]["valid?"] is True
    # the :linear member is the existing Linearizable over ledger->bank of the history
    bank = [dict(op, value=op["value"][0][2]) if op.get("f") == "transfer" else op for op in L.ledger_to_bank(h)]
    from jepsen_tigerbeetle_amd.jepsen import checker as jc
    from jepsen_tigerbeetle_amd.knossos import model as M
    assert got["linear"] == untimed(jc.Linearizable({"model": M.bank([1, 2, 3], True)}).check(None, bank))
    h2 = edn.read_history(os.path.join(ROOT, "tests", "golden", "ledger", "anomalies.edn"))
    opts2 = dict(opts, **{"negative-balances?": False})
    dev, host = L.test(opts2, device_route=True), L.test(opts2, device_route=False)
    assert dev["checker"].check(dev, h2) == host["checker"].check(host, h2)

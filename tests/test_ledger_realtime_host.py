"""The realtime bounds on the ledger's posted counters, on the CPU: the host statement `realtime_host` of jepsen/ledger.py against
hand-derived fixtures (tests/golden/ledger_realtime: one per rule and boundary, README.md there derives each), `realtime_numpy` pinned
against it on random concurrent histories, validity by construction, the planted anomalies, SOUNDNESS against the definition (no
flagged history is linearizable, by brute force over a counters model), and every ValueError."""
import glob
import json
import os
import random

import numpy as np
import pytest

import ledger_realtime_histories as G
from conftest import ROOT
from jepsen_tigerbeetle_amd.jepsen import edn
from jepsen_tigerbeetle_amd.jepsen import ledger as L
from jepsen_tigerbeetle_amd.knossos import history as H

GOLDEN = os.path.join(ROOT, "tests", "golden", "ledger_realtime")
FIXTURES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "*.json")))
ARRAYS = ("bits", "miss", "lo", "hi", "floor")


def assert_same(got, want, tag):
    for k in ARRAYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert got["summary"] == want["summary"], tag


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        want = json.load(f)
    o = dict(want["opts"])
    if "initial" in o:
        o["initial"] = {a: {"credits-posted": c, "debits-posted": d} for a, c, d in o["initial"]}
    return edn.read_history(os.path.join(GOLDEN, name + ".edn")), o, want


def test_there_is_a_fixture_per_rule_and_boundary():
    assert len(FIXTURES) == 15


@pytest.mark.parametrize("name", FIXTURES)
def test_hand_derived_fixture(name):
    h, o, want = load(name)
    got = L.realtime_host(h, o)
    for k in ARRAYS:
        assert got[k].tolist() == want[k], (name, k)
    for k, v in want["counts"].items():
        assert got["summary"][k] == v, (name, k)
    assert got["summary"]["valid"] == int(not any(want["bits"])) and got["summary"]["error_count"] == sum(b != 0 for b in want["bits"])
    if name == "value-at-int64-min":                                           # (the columns hold no read whose magnitudes reach 2^63)
        with pytest.raises(ValueError, match="reaches 2\\^63"):
            L.realtime_numpy(h, o)
    else:
        assert_same(L.realtime_numpy(h, o), got, name)
    m = L.RealtimeBounds(o).check({}, h)
    assert m["valid?"] == (not any(want["bits"])) and m["read-count"] == len(want["bits"])
    assert set(m) == {"valid?", "read-count", "error-count", "first-error", "errors"}


def test_result_map_names_reads_and_orders_violations():
    h, o, _ = load("open-transfer")
    m = L.RealtimeBounds(o).check({}, h)
    assert m["error-count"] == 1 and set(m["errors"]) == {"regressed"} and m["first-error"] == m["errors"]["regressed"]["first"]
    e = m["errors"]["regressed"]
    assert e["count"] == 1 and e["first"] == e["worst"] == e["last"] and e["first"]["op"] == dict(h[4], index=4)
    assert e["first"]["violations"] == [{"type": "regressed", "account": 1, "field": "debits-posted", "value": 0, "bound": 5},
                                        {"type": "regressed", "account": 2, "field": "credits-posted", "value": 0, "bound": 5}]
    h, o, _ = load("nonzero-initial")                                           # micro-op order, then credits before debits
    v = L.RealtimeBounds(o).check({}, h)["first-error"]["violations"]
    assert [(x["type"], x["account"], x["field"], x["value"], x["bound"]) for x in v] == [("stale", 1, "debits-posted", 10, 15), ("stale", 2, "credits-posted", 50, 55)]
    # a test map's accounts and initial override the checker's own; test() composes the member only when asked
    assert L.RealtimeBounds({}).check(o, h) == L.RealtimeBounds(o).check({}, h)
    assert "realtime" not in L.test()["checker"].checkers and "realtime" in L.test(realtime=True, device_route=False)["checker"].checkers
    res = L.test(dict(o, **{"negative-balances?": True}), realtime=True, device_route=False)["checker"].check(o, h)
    assert res["realtime"] == L.RealtimeBounds(o).check(o, h) and res["valid?"] is False


@pytest.fixture(scope="module")
def random_histories():
    out = []
    for seed in range(200):
        plant = [(), ("stale",), ("future",), ("regressed",), G.ANOMALIES][seed % 5]
        h, o, planted = G.concurrent_ledger(seed, workers=2 + seed % 5, ops=40 + seed % 30, accounts=1 + seed % 8, plant=plant)
        out.append((h, o, plant, planted, L.realtime_host(h, o)))
    return out


def test_numpy_statement_equals_host_statement(random_histories):
    flagged = 0
    for h, o, plant, planted, host in random_histories:
        assert_same(L.realtime_numpy(h, o), host, plant)
        flagged += bool(host["summary"]["error_count"])
        if host["summary"]["error_count"]:                                     # ... and so do the result maps built from either summary
            accounts, init, apply_ok = L._rt_opts(None, o)
            assert L.RealtimeBounds(o).check(o, h) == L._rt_map(h, L.realtime_numpy(h, o)["summary"], accounts, init, apply_ok)
    assert len(random_histories) >= 200 and 100 <= flagged <= 160


def test_valid_by_construction_has_no_bit_and_every_counter_within_its_bounds(random_histories):
    seen = 0
    for h, o, plant, planted, host in random_histories:
        if plant:
            continue
        assert not host["bits"].any() and not host["miss"].any() and host["summary"]["valid"] == 1
        cols = L.LedgerColumns(h)
        rd = (cols.type == L.N.LEDGER_T_OK) & (cols.kind == L.N.LEDGER_K_READ)
        m, _ = L._expand(cols.mop_off[:-1][rd].astype(np.int64), (cols.mop_off[1:][rd] - cols.mop_off[:-1][rd]).astype(np.int64))
        v = np.stack([cols.mop_a[m], cols.mop_b[m]], axis=1)
        assert host["summary"]["n_checked"] == len(m) > 0
        assert (host["lo"] <= v).all() and (v <= host["hi"]).all() and (host["floor"] <= v).all()
        assert (host["lo"] < host["hi"]).any()                                 # (the histories are concurrent: the bounds are not all tight)
        seen += 1
    assert seen == 40


def test_each_plant_sets_its_own_bit_on_the_planted_read(random_histories):
    landed = {name: 0 for name in G.ANOMALIES}
    for h, o, plant, planted, host in random_histories:
        assert set(planted) == set(plant), (plant, planted)                    # the planted read exists
        reads = list(L.LedgerColumns(h).read_ops)
        for name in plant:
            assert host["bits"][reads.index(planted[name])] & (3 << (2 * G.ANOMALIES.index(name))), (plant, name)
            landed[name] += 1
    assert all(n == 80 for n in landed.values())


# ---------------------------------------------------------------- soundness: ground truth by brute force, in the style of oracle/brute.py

def linearizable(history, init):
    """Is there an order of the operations -- every :ok op once, between its invocation and its completion; an :info or open transfer
    once at any time after its invocation, or never; a failed transfer never -- in which every :ok read returns the counters as they
    stand?  Exhaustive depth-first search; state = the counters."""
    pairs = H.pair_index(history)
    ops = []                                                                    # (inv, ret or None, must, kind, payload)
    for i, op in enumerate(history):
        if op["type"] != "invoke":
            continue
        j = pairs.get(i)
        typ = None if j is None else history[j]["type"]
        if L.op_txn_f(op) == "t":
            if typ == "fail":
                continue
            ops.append((i, j if typ == "ok" else None, typ == "ok", "t", [m[2] for m in op["value"]]))
        elif typ == "ok":
            ops.append((i, j, True, "r", history[j]["value"]))
    n = len(ops)

    def search(done, cr, db):
        if all(d or not ops[k][2] for k, d in enumerate(done)):
            return True
        horizon = min((ops[k][1] for k in range(n) if not done[k] and ops[k][1] is not None), default=None)      # the first completion still owed
        for k in range(n):
            inv, ret, must, kind, payload = ops[k]
            if done[k] or (horizon is not None and inv > horizon):
                continue
            done2 = done[:k] + (True,) + done[k + 1:]
            if kind == "t":
                cr2, db2 = dict(cr), dict(db)
                for m in payload:
                    cr2[m["credit-acct"]] += m["amount"]; db2[m["debit-acct"]] += m["amount"]
                if search(done2, cr2, db2):
                    return True
            elif all(m == {"credits-posted": cr[a], "debits-posted": db[a]} for _r, a, m in payload) and search(done2, cr, db):
                return True
        return False

    return search((False,) * n, {a: v["credits-posted"] for a, v in init.items()}, {a: v["debits-posted"] for a, v in init.items()})


def perturbed(seed):
    rng = random.Random(1000 + seed)
    h, o, _ = G.concurrent_ledger(seed, workers=3, ops=6, accounts=2, read_share=0.5, max_mops=2)
    reads = [i for i, op in enumerate(h) if op["type"] == "ok" and L.op_txn_f(op) == "r"]
    if not reads:
        return None
    i = rng.choice(reads)
    others = [h[j]["value"] for j in reads if h[j]["value"] != h[i]["value"]]
    how = rng.randrange(3)
    if how == 0 and others:
        value = rng.choice(others)                                              # another read's snapshot
    elif how == 1:
        value = [["r", a, dict(o["initial"][a])] for a in o["accounts"]]        # the initial snapshot
    else:
        value = [[r, a, dict(m)] for r, a, m in h[i]["value"]]
        value[rng.randrange(len(value))][2][rng.choice(G.FIELDS)] += rng.choice((-1, 1, 2))
    h[i] = dict(h[i], value=value)
    return h, o


def test_no_flagged_history_is_linearizable():
    total = flagged = lin = 0
    for seed in range(600):
        p = perturbed(seed)
        if p is None:
            continue
        h, o = p
        f = not L.realtime_host(h, o)["summary"]["valid"]
        g = linearizable(h, o["initial"])
        assert not (f and g), seed
        total += 1; flagged += f; lin += g
    print(f"{total} histories: {flagged} flagged, {lin} linearizable")
    assert total >= 500 and 4 * flagged >= total and 4 * lin >= total          # neither side is vacuous


def test_the_brute_force_knows_a_valid_history_from_an_invalid_one():
    for seed in range(40):
        h, o, _ = G.concurrent_ledger(seed, workers=3, ops=6, accounts=2, read_share=0.5, max_mops=2)
        assert linearizable(h, o["initial"]), seed
    h, o, _ = load("transfer-invoked-just-after-read-returns")
    assert not linearizable(h, {a: {"credits-posted": 0, "debits-posted": 0} for a in (1, 2)})


# ---------------------------------------------------------------- every ValueError

def test_every_value_error():
    h, o, _ = G.concurrent_ledger(2, ops=30, fail=0.0)
    accounts, init, apply_ok = L._rt_opts(None, o)
    t = next(i for i, op in enumerate(h) if op["type"] == "invoke" and L.op_txn_f(op) == "t")

    def with_amount(x):
        g = list(h)
        v = [[m[0], m[1], dict(m[2])] for m in h[t]["value"]]
        v[0][2]["amount"] = x
        g[t] = dict(h[t], value=v)
        return g

    for fn in (L.realtime_host, L.realtime_numpy):
        for x in (-1, 2 ** 31):
            with pytest.raises(ValueError, match="not in \\[0, 2\\^31\\)"):
                fn(with_amount(x), o)
        assert fn(with_amount(2 ** 31 - 1), o)["summary"]["read_count"]
        for x in (2 ** 61, -(2 ** 61), 1.5, True):
            with pytest.raises(ValueError, match="initial value"):
                fn(h, dict(o, initial={1: {"credits-posted": x, "debits-posted": 0}}))
        assert fn(h, dict(o, initial={1: {"credits-posted": 2 ** 61 - 1, "debits-posted": -(2 ** 61) + 1}}))["summary"]["read_count"]
    cols = L.LedgerColumns(h)
    with pytest.raises(ValueError, match="initial value"):
        L.ledger_rt_in(cols, accounts, {**init, 1: (2 ** 61, 0)}, apply_ok)
    with pytest.raises(ValueError, match="account is not an int"):
        L.ledger_rt_in(cols, [1, 2 ** 70], {1: (0, 0), 2 ** 70: (0, 0)}, apply_ok)
    with pytest.raises(ValueError, match="2\\^31 or more transfer micro-ops"):
        L._rt_ranges([], 2 ** 31, {})
    with pytest.raises(ValueError, match=":process is not an int in int32 range"):
        L.LedgerColumns([dict(h[0], process=2 ** 31)] + h[1:])
    assert L.LedgerColumns(h).process.dtype == np.int32 and len(L.LedgerColumns(h).process) == len(L.LedgerColumns(h))

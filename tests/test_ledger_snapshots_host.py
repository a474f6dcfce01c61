"""The snapshot order of a ledger's reads, on the CPU: `snapshots_numpy` (sort and scan, what the device is held to) pinned against the
O(R^2) specification `snapshots_host` of jepsen/ledger.py on random vector sets with partial reads, negative values and equal sums; the
EQUIVALENCE with the cycle search -- complete reads, a plain DFS over monotonic-key + realtime edges: acyclic exactly when no read is
skewed and none has a regressed bit --; concurrent ledgers, on which the realtime plants leave no skew (they substitute other TRUE
snapshots: the two checkers are orthogonal) and a fork leaves :SI and the realtime bounds valid and the snapshot order invalid; the range
error, the result map and test(snapshots=True)."""
import random

import numpy as np
import pytest

import ledger_realtime_histories as G
import ledger_snapshot_histories as S
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

ARRAYS = ("count", "first", "key", "flags")


def assert_same(got, want, tag):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert got["summary"] == want["summary"], tag


def test_numpy_statement_equals_the_specification_on_random_vectors():
    rng = random.Random(3)
    seen_partial = seen_skew = seen_atomic = 0
    for trial in range(150):
        accounts = rng.sample(range(1, 40), rng.choice((1, 2, 3, 5)))
        h, o = S.reads_ledger(accounts, S.random_rows(rng, accounts, rng.randint(0, 14)))
        want, got = L.snapshots_host(h, o), L.snapshots_numpy(h, o)
        assert_same(got, want, trial)
        seen_partial += want["summary"]["n_partial"] > 0
        seen_skew += want["summary"]["n_pairs"] > 0
        seen_atomic += want["summary"]["skewed"]["count"] > want["summary"]["n_candidates"]
    assert seen_partial > 50 and seen_skew > 50 and seen_atomic > 0


def test_shape_cases_have_the_shape_they_were_built_for():
    for case in S.shape_cases(big=False):
        want = L.snapshots_numpy(case["history"], case["opts"])
        for k, v in case["counts"].items():
            assert (want["summary"]["skewed"]["count"] if k == "skewed" else want["summary"][k]) == v, (case["name"], k)
        if want["summary"]["read_count"] <= 130:
            assert_same(want, L.snapshots_host(case["history"], case["opts"]), case["name"])


def _acyclic(n, edges):
    state = [0] * n

    def visit(u):
        state[u] = 1
        for v in edges[u]:
            if state[v] == 1 or (state[v] == 0 and not visit(v)):
                return False
        state[u] = 2
        return True

    return all(state[u] or visit(u) for u in range(n))


def test_no_skew_and_no_regression_is_exactly_an_acyclic_graph():
    """complete reads, at most 7: the graph has an edge R -> R' where R is below R' on some counter (monotonic keys) and where R completed
    before R' was invoked (real time)"""
    rng = random.Random(9)
    acyclic = 0
    for trial in range(400):
        accounts = [1] if rng.random() < 0.5 else [1, 2]
        n = rng.randint(1, 7)
        values = [[["r", a, {"credits-posted": rng.randint(0, 2), "debits-posted": rng.randint(0, 2)}] for a in accounts] for _ in range(n)]
        steps = [(k, t) for k in range(n) for t in ("invoke", "ok")]
        rng.shuffle(steps)
        hist, inv, ret = [], {}, {}
        open_ = set()
        order = []
        for k, _t in steps:                                                    # a read's first step invokes it, its second completes it
            order.append((k, "ok" if k in open_ else "invoke"))
            open_.add(k)
        for k, t in order:
            S._op(hist, k, t, [["r", a, None] for a in accounts] if t == "invoke" else values[k])
            (inv if t == "invoke" else ret)[k] = len(hist) - 1
        o = {"accounts": accounts}
        numbered = sorted(range(n), key=lambda k: ret[k])                      # read numbers: by completion
        vec = [[m[f] for _r, _a, m in values[k] for f in S.FIELDS] for k in numbered]
        edges = [[v for v in range(n) if v != u and (any(x < y for x, y in zip(vec[u], vec[v])) or ret[numbered[u]] < inv[numbered[v]])] for u in range(n)]
        snap, rt = L.snapshots_numpy(hist, o), L.realtime_host(hist, o)
        assert snap["summary"]["n_partial"] == 0
        no_anomaly = snap["summary"]["valid"] == 1 and not (rt["bits"] & 48).any()
        assert _acyclic(n, edges) == no_anomaly, trial
        acyclic += no_anomaly
    assert 20 < acyclic < 380


@pytest.mark.parametrize("plant", [(), ("stale",), ("future",), ("regressed",)])
def test_concurrent_ledgers_and_the_realtime_plants_hold_no_skew(plant):
    """a read of a concurrent ledger is a true snapshot, and every realtime plant substitutes ANOTHER true snapshot (the initial one, the
    final one, an earlier read's): the snapshot order cannot see them, as the realtime bounds cannot see a fork"""
    for seed in range(6):
        h, o, planted = G.concurrent_ledger(200 + seed, workers=6, ops=160, plant=plant)
        assert set(planted) == set(plant)
        got = L.snapshots_numpy(h, o)
        assert got["summary"]["valid"] == 1 and got["summary"]["n_partial"] == 0 and got["summary"]["n_candidates"] == 0, (plant, seed)
        assert not got["count"].any() and got["summary"]["read_count"] > 20
        assert L.RealtimeBounds(o).check(o, h)["valid?"] == (not plant)


def test_a_fork_passes_every_other_checker():
    for seed in range(4):
        h, o, planted = S.forked_ledger(300 + seed, forks=1 + seed % 2, workers=5, ops=120)
        assert L.RealtimeBounds(o).check(o, h)["valid?"] is True
        assert L.BankChecker(o).check(o, h)["valid?"] is True
        m = L.SnapshotOrder(o).check(o, h)
        assert m["valid?"] is False and m["exact?"] is True and m["pair-count"] == 1 + seed % 2 and m["skewed-count"] == 2 * (1 + seed % 2)
        assert m["first"]["op"]["index"] == planted["R"][0] and m["first"]["with"]["index"] == planted["R2"][0]
        assert m["last"]["op"]["index"] == planted["R2"][-1] and m["worst"] == m["first"]
        got = L.snapshots_numpy(h, o)
        assert_same(got, L.snapshots_host(h, o), seed)
        assert got["summary"]["n_candidates"] == 2 * (1 + seed % 2)


def test_a_torn_read_is_skewed_and_its_total_holds():
    h, o, r = S.torn_ledger(32, workers=5, ops=150)
    assert L.BankChecker(o).check(o, h)["valid?"] is True
    got = L.snapshots_numpy(h, o)
    assert_same(got, L.snapshots_host(h, o), "torn")
    cols = L.LedgerColumns(h)
    assert got["count"][list(cols.read_ops).index(r)] > 0 and got["summary"]["valid"] == 0


def test_the_result_map_names_ops_and_counters():
    accounts = [3, 1]
    h, o = S.reads_ledger(accounts, [[(3, 9, 9), (1, 9, 9)], [(3, 5, 5), (1, 5, 6)], [(3, 5, 5), (1, 6, 5)], [(1, 7, 4)]], transfers_first=2)
    m = L.SnapshotOrder(o).check({}, h)
    assert set(m) == {"valid?", "exact?", "read-count", "partial-count", "skewed-count", "pair-count", "first", "worst", "last"}
    assert (m["valid?"], m["exact?"], m["read-count"], m["partial-count"], m["skewed-count"], m["pair-count"]) == (False, False, 4, 1, 3, 3)
    reads = [i for i, op in enumerate(h) if op["type"] == "ok" and op["value"][0][0] == "r"]
    assert m["first"] == {"op": h[reads[1]], "skew-count": 2, "with": h[reads[2]], "below": [1, "credits-posted"], "above": [1, "debits-posted"]}
    assert m["worst"] == m["first"]                                            # (three reads of count 2: the earliest)
    assert m["last"] == {"op": h[reads[3]], "skew-count": 2, "with": h[reads[1]], "below": [1, "debits-posted"], "above": [1, "credits-posted"]}
    cols = L.LedgerColumns(h)
    assert L.snapshots_result_map(h, cols, L.snapshots_numpy(h, o), accounts) == m
    valid = L.SnapshotOrder(o).check({}, h[:6])
    assert valid == {"valid?": True, "exact?": True, "read-count": 1, "partial-count": 0, "skewed-count": 0, "pair-count": 0, "first": None, "worst": None, "last": None}
    assert L.SnapshotOrder({"accounts": [3]}).check({"accounts": accounts}, h) == m      # (the test map's accounts win)


def test_magnitudes_that_reach_2_to_the_63_are_refused():
    big = {"credits-posted": 2 ** 62, "debits-posted": 2 ** 62}
    h, o = S.reads_ledger([1], [[(1, 1, 1)]])
    h[-1] = dict(h[-1], value=[["r", 1, big]])
    with pytest.raises(ValueError, match="2\\^63"):
        L.snapshots_host(h, o)
    with pytest.raises(ValueError, match="2\\^63"):
        L.SnapshotOrder(o).check({}, h)
    with pytest.raises(ValueError, match="2\\^63"):
        L.snapshots_numpy(h, o)                                                # (LedgerColumns refuses it)
    V, K = np.array([[2 ** 62, 2 ** 62], [-(2 ** 62), 2 ** 62 - 1]], np.int64), np.ones((2, 2), bool)
    with pytest.raises(ValueError, match="2\\^63"):
        L.snapshots_dense_numpy(V, K)
    assert L.snapshots_dense_numpy(V[1:], K[1:])["summary"]["valid"] == 1
    K[0, 1] = False                                                            # an unchecked counter does not count
    assert L.snapshots_dense_numpy(V, K)["summary"]["n_partial"] == 1
    # a foreign id's values are not checked either: the host statement takes the read
    h[-1] = dict(h[-1], value=[["r", 1, {"credits-posted": 1, "debits-posted": 1}], ["r", 99, {"credits-posted": 2 ** 62, "debits-posted": 0}]])
    assert L.snapshots_host(h, o)["summary"]["valid"] == 1


def test_the_composed_member_on_the_host_route():
    h, o, planted = S.forked_ledger(41, workers=4, ops=80)
    res = L.test(o, realtime=True, snapshots=True, device_route=False)["checker"].check(o, h)
    assert res["snapshots"]["valid?"] is False and res["valid?"] is False
    assert all(res[k]["valid?"] is True for k in ("SI", "realtime")) and res["snapshots"] == L.SnapshotOrder(o).check(o, h)
    assert "snapshots" not in L.test(o, device_route=False)["checker"].check(o, h)
    assert N.LEDGER_SNAP_PARTIAL == L.SNAP_PARTIAL and N.LEDGER_SNAP_SKEWED == L.SNAP_SKEWED

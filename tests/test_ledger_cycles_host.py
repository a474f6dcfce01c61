"""The cycle search over the ledger's reads on the host (jepsen/ledger.py "Cycle search"): cycles_host -- the explicit graph and Tarjan,
the truth -- against cycles_numpy, the reduction the device computes, on every curated history of tests/ledger_cycle_histories.py and
on a few thousand random ones; what a cycle means on all-complete histories (the snapshot rule plus the regressed bit, exactly) and on
every history (a skewed or regressed read is on a cycle; a skewed pair shares a label); the checker, its result map and its witness."""
import random

import numpy as np
import pytest

import ledger_cycle_histories as CH
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

CASES = CH.cases()


def assert_same(got, want, tag, rounds=True):
    for k in L.CYC_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    drop = ("ns_device", "bytes_in") + (() if rounds else ("closure_rounds",))
    assert {k: v for k, v in got["summary"].items() if k not in drop} == {k: v for k, v in want["summary"].items() if k not in drop}, tag


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reduction_equals_specification_on_curated_histories(case):
    h, o = case["history"], case["opts"]
    got = L.cycles_numpy(h, o)
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert got["summary"][k] == v, (case["name"], k)
    assert_same(got, L.cycles_host(h, o), case["name"], rounds=False)
    m = got["summary"]["n_core"]
    assert got["summary"]["closure_rounds"] <= (int(np.ceil(np.log2(m))) + 1 if m else 0)


def test_reduction_equals_specification_on_random_histories():
    rng = random.Random(5)
    seen = {"cycle": 0, "clean read on a cycle": 0, "valid with a core": 0, "no invocation": 0, "checks nothing": 0}
    for trial in range(3000):
        h, o = CH.random_history(rng)
        got = L.cycles_numpy(h, o)
        assert_same(got, L.cycles_host(h, o), (trial, h, o), rounds=False)
        s, f = got["summary"], got["flags"]
        seen["cycle"] += s["n_on_cycle"] > 0
        seen["clean read on a cycle"] += bool(((f & (L.CYC_ON_CYCLE | L.CYC_CORE)) == L.CYC_ON_CYCLE).any())
        seen["valid with a core"] += s["valid"] and s["n_core"] > 0
        seen["no invocation"] += sum(op["type"] == "ok" for op in h) > sum(op["type"] == "invoke" for op in h)
        seen["checks nothing"] += s["n_checked"] < sum(len(op["value"]) for op in h if op["type"] == "ok")
    assert all(v >= 100 for v in seen.values()), seen


def _anomalies(h, o):
    skew = L.snapshots_host(h, o)
    rt = L.realtime_host(h, o)
    return skew, (skew["count"] > 0) | ((rt["bits"] & 48) != 0)


def test_all_complete_histories_cycle_exactly_when_skewed_or_regressed():
    rng = random.Random(9)
    n = {True: 0, False: 0}
    for trial in range(1500):
        h, o = CH.random_history(rng)
        got = L.cycles_host(h, o)
        if got["summary"]["n_partial"]:
            continue
        _skew, bad = _anomalies(h, o)
        assert bool(got["summary"]["n_on_cycle"]) == bool(bad.any()), (trial, h, o)
        n[bool(bad.any())] += 1
    assert min(n.values()) >= 50, n


def test_skewed_and_regressed_reads_are_on_cycles_and_skewed_pairs_share_a_label():
    rng = random.Random(10)
    pairs = 0
    for trial in range(1500):
        h, o = CH.random_history(rng)
        got = L.cycles_host(h, o)
        skew, bad = _anomalies(h, o)
        assert ((got["flags"][bad] & L.CYC_ON_CYCLE) != 0).all(), (trial, h, o)
        for r in np.flatnonzero(skew["count"]):
            assert got["scc"][r] == got["scc"][skew["first"][r]] != N.NO_OP
            pairs += 1
    assert pairs >= 500


def test_the_three_partial_cycle_is_what_no_other_member_decides():
    case = next(c for c in CASES if c["name"] == "three-partial-cycle")
    h, o = case["history"], case["opts"]
    snap = L.SnapshotOrder(o).check({}, h)
    assert snap["valid?"] is True and snap["exact?"] is False
    assert not (L.realtime_host(h, o)["bits"] & 48).any() and not L.snapshots_host(h, o)["count"].any()     # no read regressed, no pair skewed
    res = L.CycleSearch(o).check({}, h)
    assert res["valid?"] is False and res["exact?"] is True and res["on-cycle-count"] == 3 and res["component-count"] == 1
    assert [c["size"] for c in res["components"]] == [3] and res["components"][0]["label"] == h[3]
    w = res["witness"]
    assert [s["type"] for s in w] == ["monotonic"] * 3 and w[0]["from"] == h[3] and w[-1]["to"] == h[3]
    assert all(a["to"] == b["from"] for a, b in zip(w, w[1:]))
    assert w[0]["key"] == [2, "credits-posted"] and (w[0]["value"], w[0]["value'"]) == (1, 2)


def test_result_maps_of_both_statements_agree_and_witnesses_are_cycles():
    for case in CASES:
        h, o = case["history"], case["opts"]
        host = L.CycleSearch(o).check({}, h)
        assert host == L._cyc_map(h, L.cycles_numpy(h, o), o["accounts"]), case["name"]
        if host["valid?"]:
            assert host["components"] == [] and host["witness"] is None
            continue
        w = host["witness"]
        assert 2 <= len(w) <= host["components"][0]["size"] and w[0]["from"] == w[-1]["to"] == host["components"][0]["label"]
        assert all(a["to"] == b["from"] for a, b in zip(w, w[1:])) and {s["type"] for s in w} <= {"realtime", "monotonic"}
        assert len(host["components"]) == min(10, host["component-count"]) and all(len(c["ops"]) == min(10, c["size"]) for c in host["components"])


def test_the_composed_test_has_the_member():
    case = next(c for c in CASES if c["name"] == "through-clean-reads")
    t = L.test(dict(case["opts"]), device_route=False, cycles=True)
    assert t["checker"].check(t, case["history"], {})["cycles"]["valid?"] is False
    assert "cycles" not in L.test(dict(case["opts"]), device_route=False)["checker"].check(t, case["history"], {})


def test_values_out_of_range_are_refused():
    h, o = CH.concurrent([1, 2], [[(1, 2 ** 62, 2 ** 62), (2, 0, 0)], [(1, 1, 1)]])
    for f in (L.cycles_host, L.cycles_numpy):
        with pytest.raises(ValueError):
            f(h, o)

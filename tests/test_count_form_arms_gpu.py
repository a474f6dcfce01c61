"""Every pass of the count form AFTER ITS BUDGET on the MI355X against oracle/wgl.py check_count_pipeline, through the C-ABI: the curated
histories of tests/count_form_arms.py (tests/test_count_form_arms_oracle.py pins them on the CPU) one at a time, through tbc_check with
the relaxed sweep in front, in batches that hold several arms at once, in the narrow kernel, as fresh inputs and with a witness.  Every
comparison is exact: verdict, failing op, the op before it, probes / visited / backtracks summed over the passes, final state, witness,
and the one config an INVALID verdict of a linearizable prefix comes with.  Nothing is planted on the device."""
import numpy as np
import pytest

import count_form_arms as A
from helpers import op_tuples
from jepsen_tigerbeetle_amd import _native as N, core
from oracle import brute

pytestmark = pytest.mark.gpu

KEYS = ("valid", "fail_op", "prev_ok_op", "probes", "visited", "backtracks", "final_state", "search_width")
DFS = [c for c in A.CASES if not c.sweep]
SWEPT = [c for c in A.CASES if c.sweep]


def _id(c):
    return f"{c.hist}-w{c.width}-rp{c.round_pairs}{'-sweep' if c.sweep else ''}"


def gm():
    return core.make_model(N.MODEL_CAS_REGISTER, N.NIL)


def opts(width=0, round_pairs=64, want_witness=False):
    """the schedule named (search_width, or lanes_per_history for the narrow kernel: no sweep) or, width 0, the library's defaults"""
    kw = {} if width == 0 else dict(lanes_per_history=round_pairs) if width == 1 else dict(search_width=width)
    return core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, count_form=True, want_witness=want_witness, **kw)


def keys(res):
    return [tuple(r[k] for k in KEYS) for r in res]


def assert_answer(g, e, tag, narrow=False, witness=False, hist=None):
    assert g["valid"] != N.UNKNOWN, (tag, g["cause"])
    assert g["valid"] == e["valid"], (tag, e["arm"], g["valid"])
    assert (g["probes"], g["visited"], g["backtracks"]) == (e["probes"], e["visited"], e["backtracks"]), (tag, e["arm"])
    if e["valid"] == 0:
        assert g["fail_op"] == e["fail_op"], (tag, e["arm"])
        if "relaxed" in e["arm"] or "prefix" in e["arm"]:
            assert g["prev_ok_op"] == e["prev"], (tag, e["arm"], g["prev_ok_op"], e["prev"])
        if e["arm"].endswith("prefix"):          # (the comment above count_form_pipeline: the one config the prefix's linearization ended in)
            if narrow:
                assert g["configs"] == [], (tag, e["arm"])
            else:
                assert len(g["configs"]) == 1 and g["configs"][0]["state"] == e["prefix_state"], (tag, e["arm"], g["configs"])
    else:
        assert g["final_state"] == e["final_state"], (tag, e["arm"])
        if witness:
            assert np.array_equal(g["witness"], e["witness"]), tag
            assert brute.check_witness(A.CAS, op_tuples(A.history(hist)), [int(x) for x in g["witness"]]) == g["final_state"], tag


def assert_regrown(c, g):
    """a line of A.REGROWN: a pass after the budget filled the first size of its visited set and was taken again with one 16 times the
    size (tests/test_count_form_arms_oracle.py: which pass -- none of them carries a prefix target)"""
    if (c.hist, c.width, c.sweep) in A.REGROWN:
        assert g["table_slots"] == 16 * A.first_table_size(A.history(c.hist)), (_id(c), g["table_slots"])


def run_twice(hists, o):
    with core.Batch(hists, gm(), o) as b:
        res = b.run().results()
        again = b.run().results()
        lanes, width = b.lanes_per_history(), b.search_width()
    assert keys(again) == keys(res)
    return res, lanes, width


# ---- (a) one history, depth-first route
@pytest.mark.parametrize("c", DFS, ids=_id)
def test_one_history_past_its_budget_on_a_named_schedule(native, oracle, c):
    e = A.expected(oracle, c.hist, c.width, c.round_pairs)
    assert e["arm"] == c.arm
    res, lanes, width = run_twice([A.history(c.hist)], opts(c.width, c.round_pairs))
    assert (lanes, width) == ((c.round_pairs, 1) if c.width == 1 else (64, c.width))
    assert_answer(res[0], e, _id(c), narrow=c.width == 1)
    assert_regrown(c, res[0])


# ---- (b) one history, sweep route: tbc_check with the library's defaults
@pytest.mark.parametrize("c", SWEPT, ids=_id)
def test_one_history_through_tbc_check_with_the_relaxed_sweep_in_front(native, oracle, c):
    g = core.check_ops(A.history(c.hist), gm(), opts())
    e = A.expected(oracle, c.hist, g["search_width"], 64, sweep=True)
    assert e["arm"] == c.arm and g["search_width"] == c.width == A.default_width([A.history(c.hist)])
    assert_answer(g, e, _id(c))
    assert_regrown(c, g)


@pytest.mark.parametrize("name", A.SWEEP_GIVES_UP)
def test_a_relaxed_sweep_that_outgrows_its_sets_leaves_the_history_to_the_depth_first_passes(native, oracle, name):
    """exhausted-b through tbc_check: the oracle's relaxed sweep refutes it (check_count_pipeline(relaxed_sweep=True): one prefix pass,
    40,154 probes, 19,367 visited), the kernel's does not conclude -- its bursts outgrow the sets -- and the library answers by the
    pipeline WITHOUT the sweep: budgeted, relaxed depth-first, prefix -- (probes, visited, backtracks) = (250976, 98026, 97770) at width 2,
    the same verdict and failing op."""
    g = core.check_ops(A.history(name), gm(), opts())
    swept = A.expected(oracle, name, g["search_width"], 64, sweep=True)
    e = A.expected(oracle, name, g["search_width"], 64)
    assert (e["valid"], e["fail_op"]) == (swept["valid"], swept["fail_op"]) and e["probes"] != swept["probes"]
    assert_answer(g, e, name)


# ---- (c), (d) mixed batches: several arms at once in pend / pend_dfs / longer / prefix / targets and in the groups of budgeted_pass
def mixed_expected(oracle, names, width, round_pairs, sweep=False, want_witness=False):
    longest = max(len(A.history(n)) for n in names)
    return [A.expected(oracle, n, width, round_pairs, sweep, longest, want_witness) for n in names]


@pytest.mark.parametrize("width,round_pairs", [(4, 64), (1, 8), (1, 16)])
def test_a_depth_first_batch_of_every_arm_at_once(native, oracle, width, round_pairs):
    names = A.MIXED_DFS
    exp = mixed_expected(oracle, names, width, round_pairs)
    arms = {(e["arm"], e["valid"]) for e in exp}
    assert arms >= set(A.DFS_ARMS) and any(a == "exact" for a, _ in arms), arms          # (recomputed under the batch's budget: every arm is still there)
    res, lanes, w = run_twice([A.history(n) for n in names], opts(width, round_pairs))
    assert (lanes, w) == ((round_pairs, 1) if width == 1 else (64, 4))
    for n, g, e in zip(names, res, exp):
        assert_answer(g, e, (n, width, round_pairs), narrow=width == 1)


def test_a_sweep_route_batch_of_every_arm_at_once(native, oracle):
    names = A.MIXED_SWEEP
    assert len(names) <= 8
    hists = [A.history(n) for n in names]
    res, lanes, width = run_twice(hists, opts())
    assert (lanes, width) == (64, A.default_width(hists))
    exp = mixed_expected(oracle, names, width, 64, sweep=True)
    assert {e["arm"] for e in exp} >= {"relaxed sweep", "relaxed sweep, prefix", "relaxed sweep, prefix exhausted", "exact, no budget", "exact"}
    assert {e["valid"] for e in exp if e["arm"] == "exact, no budget"} == {0, 1}
    for n, g, e in zip(names, res, exp):
        assert_answer(g, e, n)


# ---- (e) fresh inputs whose histories go past the budget
@pytest.mark.parametrize("width,round_pairs", [(4, 64), (1, 8)])
def test_a_fresh_input_goes_past_the_budget(native, oracle, width, round_pairs):
    calm, names = [A.history(h) for h in A.CALM], A.MIXED_DFS
    mixed = [A.history(n) for n in names]
    exp_calm = [A.expected(oracle, h, width, round_pairs, False, max(len(x) for x in calm)) for h in A.CALM]
    exp_mixed = mixed_expected(oracle, names, width, round_pairs)
    assert all(e["arm"] == "exact" for e in exp_calm)
    o = opts(width, round_pairs)
    with core.Batch(mixed, gm(), o) as fresh:
        created = keys(fresh.run().results())
    with core.Batch(calm, gm(), o) as b:
        first = b.run().results()
        for i, (g, e) in enumerate(zip(first, exp_calm)):
            assert_answer(g, e, ("calm", i), narrow=width == 1)
        b.reload(mixed)
        second = b.run().results()
        for n, g, e in zip(names, second, exp_mixed):
            assert_answer(g, e, ("reloaded", n), narrow=width == 1)
        assert keys(second) == created
        assert b.input_info()["inputs_consumed"] == 1
        b.reload(calm)
        third = b.run().results()
        assert keys(third) == keys(first)
        for i, (g, e) in enumerate(zip(third, exp_calm)):
            assert_answer(g, e, ("calm again", i), narrow=width == 1)


# ---- (f) with a witness
def test_the_late_passes_with_a_witness(native, oracle):
    names = [c.hist for c in DFS if c.width == 4 and (c.arm, c.valid) == ("exact, no budget", 1)] + ["prefix-a", "stale-a", "exhausted-a"]
    assert len(names) >= 5
    for n in names:
        e = A.expected(oracle, n, 4, 64, want_witness=True)
        plain = A.expected(oracle, n, 4, 64)
        assert (e["arm"], e["valid"], e["fail_op"], e["probes"]) == (plain["arm"], plain["valid"], plain["fail_op"], plain["probes"]) and e["arm"] != "exact"
        with core.Batch([A.history(n)], gm(), opts(4, want_witness=True)) as b:
            g = b.run().results()[0]
        assert_answer(g, e, n, witness=True, hist=n)

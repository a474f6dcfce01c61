"""TBC_MODEL_MUTEX and TBC_MODEL_TABLE (the memo table: the bank that forbids overdrafts, a set with repeated adds) on every device
engine that takes them, against the oracle of that engine's schedule: the sequential kernel (wgl_search.hip), the wide kernel
(wgl_beam.hip: the register-family instance for the mutex, the generic one for the table), several histories per wavefront (mutex
only), the level sweep (jit_sweep.hip), fresh inputs (batch_stream.hip), the shipped defaults and the knossos surface.  The histories,
their shapes and the sequential reference are tests/model_histories.py's (computed once, shared); the oracles themselves are pinned
against brute force in tests/test_models_oracle.py.  No case is left out of a comparison: every reference must finish (asserted)."""
import numpy as np
import pytest

import model_histories as MH
from helpers import _assert_narrow, assert_same
from jepsen_tigerbeetle_amd import _native as N, core
from jepsen_tigerbeetle_amd.knossos import competition, linear, model as M, wgl
from oracle import brute

pytestmark = pytest.mark.gpu

GROUPS = ("mutex", "mutex-held", "table", "set-table")          # one tbc_model each: what may share a batch
KEYS = ("valid", "fail_op", "prev_ok_op", "probes", "visited", "backtracks", "max_depth", "steps", "final_state")      # (tests/test_stream_gpu.py's)


def names_of(group, mw=None):
    return [s[0] for s in MH.SHAPES if s[1] == group and (mw is None or s[2] == mw)]


def opts(**kw):
    return core.make_opts(time_limit_ms=60000, **kw)


def replay(c, got, tag):
    assert brute.check_witness(c.om, c.tuples(), [int(x) for x in got["witness"]]) == got["final_state"], tag


# ---- the sequential kernel
@pytest.mark.parametrize("group", GROUPS)
def test_sequential_kernel_matches_the_window_oracle(native, oracle, group):
    """TBC_ALG_WGL: every shape of the model (1, 2, 4 and more mask words; crashed calls; valid and not), one history at a time and
    all of them as one batch: verdict, failing op, the op before it, final state, witness and every counter."""
    cases = MH.references(oracle, names_of(group))
    o = opts(algorithm=N.ALG_WGL)
    for c in cases:
        got = core.check_ops(c.ops, c.native, o)
        assert got["search_width"] == 1, c.name
        assert_same(got, c.ref, c.name)
        if c.ref["valid"] == 1:
            replay(c, got, c.name)
    with core.Batch([c.ops for c in cases], cases[0].native, o) as b:
        res = b.run().results()
    for c, got in zip(cases, res):
        assert_same(got, c.ref, ("batch", c.name))


@pytest.mark.parametrize("group", ["mutex", "table"])
def test_more_than_256_slots_go_to_the_sequential_kernel(native, oracle, group):
    """knossos.competition over a history with more than four mask words: plan_engines gives it the sequential kernel, same numbers."""
    for c in MH.references(oracle, [group + "-8", group + "-8-bad"], seeds=(0,)):
        assert c.ops.n_process > 256
        got = core.check_ops(c.ops, c.native, opts(algorithm=N.ALG_COMPETITION))
        assert got["search_width"] == 1, c.name
        assert_same(got, c.ref, c.name)


# ---- the wide kernel
@pytest.mark.parametrize("mw", [1, 2, 4])
@pytest.mark.parametrize("width", [2, 8, 16])
@pytest.mark.parametrize("model", ["mutex", "table"])
def test_wide_kernel_matches_its_oracle(native, oracle, model, width, mw):
    """search_width 2 / 8 / 16 x 1 / 2 / 4 mask words, one launch each (at one mask word a second one for the model's other start: the
    mutex held at the start, the set's table): against oracle/wgl_beam.c at that width (no rules, no lookahead for these models) --
    verdict, failing op, the op before it, final state, witness, every counter; the witness replayed; one history again alone."""
    o = opts(algorithm=N.ALG_COMPETITION, search_width=width)
    for group in ([model] if mw > 1 else [model, "mutex-held" if model == "mutex" else "set-table"]):
        cases = MH.references(oracle, names_of(group, mw))
        assert cases and any(c.crashed for c in cases) and {c.ref["valid"] for c in cases} == {0, 1}, group
        with core.Batch([c.ops for c in cases], cases[0].native, o) as b:
            assert b.search_width() == width and b.lanes_per_history() == 64
            res = b.run().results()
        for c, got in zip(cases, res):
            exp = oracle.check_beam(c.d(), c.om, width, max_probes=MH.MAX_PROBES)
            assert exp["valid"] != -1, c.name
            assert (exp["valid"], exp["fail_op"] if exp["valid"] == 0 else None) == (c.ref["valid"], c.ref["fail_op"] if c.ref["valid"] == 0 else None), c.name
            assert got["valid"] == exp["valid"] and got["search_width"] == width, (c.name, got["valid"], got["cause"])
            if exp["valid"] == 0:
                assert got["fail_op"] == exp["fail_op"], c.name
                assert got["prev_ok_op"] == (None if exp["prev_ok_op"] == N.NO_OP else exp["prev_ok_op"]), c.name
            else:
                assert got["final_state"] == exp["final_state"], c.name
                assert np.array_equal(got["witness"], exp["witness"]), c.name
                replay(c, got, c.name)
            assert (got["probes"], got["visited"], got["backtracks"], got["max_depth"]) == \
                   (exp["probes"], exp["visited"], exp["expanded"], exp["max_stack"]), c.name
        k = len(cases) // 2
        single = core.check_ops(cases[k].ops, cases[k].native, o)
        assert [single[x] for x in KEYS] == [res[k][x] for x in KEYS], cases[k].name
        assert single["valid"] != 1 or np.array_equal(single["witness"], res[k]["witness"])


# ---- several histories per wavefront: mutex only
@pytest.mark.parametrize("L,mw", [(8, 1), (16, 1), (32, 1), (8, 2), (16, 2), (8, 4)])
def test_narrow_kernel_mutex_matches_its_oracle(native, oracle, L, mw):
    """lanes_per_history = L: every mutex shape of that mask width x 3 seeds in ONE launch, run twice (the same answers), each on the
    oracle's schedule of one config per iteration and L pairs per round.  At two and four mask words this is the regression test of
    the front records: a batch without rule tables (a mutex has no register values) used to have them packed in the compact form
    that only the one-word kernel reads."""
    groups = ["mutex"] + (["mutex-held"] if (L, mw) == (8, 1) else [])
    for group in groups:
        cases = MH.references(oracle, names_of(group, mw), seeds=(0, 1, 2))
        with core.Batch([c.ops for c in cases], cases[0].native, opts(algorithm=N.ALG_COMPETITION, lanes_per_history=L)) as b:
            assert b.lanes_per_history() == L and b.search_width() == 1
            res = b.run().results()
            again = b.run().results()
        for c, got, g2 in zip(cases, res, again):
            exp = oracle.check_beam(c.d(), c.om, 1, round_pairs=L, rules_at_any_round_size=True, branch_lists=True, max_probes=MH.MAX_PROBES)
            assert exp["valid"] != -1 and exp["valid"] == c.ref["valid"], c.name
            _assert_narrow(got, exp, (L, c.name))
            if exp["valid"] == 0:
                assert got["fail_op"] == c.ref["fail_op"], c.name
            else:
                replay(c, got, c.name)
            assert [g2[x] for x in KEYS] == [got[x] for x in KEYS], c.name


def test_narrow_kernel_refuses_the_table_by_name(native, oracle):
    cases = MH.references(oracle, ["table-1", "table-1-bad"])
    with pytest.raises(N.TbcError) as e:
        core.Batch([c.ops for c in cases], cases[0].native, opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8))
    assert e.value.status == N.ERR_UNSUPPORTED


# ---- the level sweep
SWEEP_SHAPES = {"mutex": ["mutex-1", "mutex-1-bad", "mutex-1-crashes-bad", "mutex-sweep-crashes"],
                "mutex-held": ["mutex-held-1", "mutex-held-1-bad"],
                "table": ["table-1", "table-1-bad", "table-sweep-crashes", "table-1-crashes-bad"],
                "set-table": ["set-table", "set-table-bad"]}


@pytest.mark.parametrize("group", GROUPS)
def test_level_sweep_matches_its_oracle(native, oracle, group):
    """TBC_ALG_LINEAR without a witness, one segment per history (plan_sweep_segments cuts the register family only): verdict and
    failing op are the sequential oracle's, the statistics oracle/sweep_ref.c's.  The shapes keep every level within the smallest
    LDS sets (512 configs) and at most 64 calls open, so EVERY history must be answered by the sweep itself."""
    cases = MH.references(oracle, SWEEP_SHAPES[group])
    assert all(c.ops.n_process <= 64 and c.peak <= 64 for c in cases)
    with core.Batch([c.ops for c in cases], cases[0].native, opts(algorithm=N.ALG_LINEAR, want_witness=False)) as b:
        res = b.run().results()
        info = b.sweep_info()
        again = b.run().results()
    assert info["enabled"] == 1 and info["seg_target"] == 0 and info["max_segs"] == 1 and info["n_fallback"] == 0, info
    for c, got, g2 in zip(cases, res, again):
        exp = oracle.check_sweep(c.d(), c.om, seg_target=info["seg_target"], n_dom=info["n_dom"])
        assert exp["valid"] != -1 and exp["max_level"] <= 512, (c.name, exp["max_level"])
        assert (exp["valid"], exp["fail_op"] if exp["valid"] == 0 else None) == (c.ref["valid"], c.ref["fail_op"] if c.ref["valid"] == 0 else None), c.name
        assert got["analyzer"] == N.ALG_LINEAR, (c.name, "handed to the depth-first search")
        assert got["valid"] == exp["valid"], c.name
        if exp["valid"] == 0:
            assert got["fail_op"] == exp["fail_op"], c.name
            assert got["prev_ok_op"] == (None if exp["prev_ok_op"] == N.NO_OP else exp["prev_ok_op"]), c.name
            assert got["configs"], c.name
        assert (got["visited"], got["probes"], got["backtracks"], got["max_depth"]) == \
               (exp["configs_total"], exp["probes"], exp["subrounds"], exp["max_level"]), c.name
        assert (g2["valid"], g2["fail_op"], g2["visited"], g2["probes"]) == (got["valid"], got["fail_op"], got["visited"], got["probes"]), c.name


# ---- fresh inputs
def _mutex_set(seed0, count, n_ops=300, info=0.0, bad_every=5):
    """mutex histories of several lengths with an all-nil value column (the wire format's 0xFF), every bad_every-th one corrupted"""
    out = []
    for s in range(count):
        hist = MH.mutex_history(n_ops + 17 * (s % 7), 8, seed0 + s, busy=0.5, info=info, corrupt=MH.MUTEX_CORRUPT if bad_every and s % bad_every == 0 else None)
        o = MH.encode_mutex(hist)[0].ops
        o.a[:] = N.NIL
        out.append(o)
    return out


def _key(r):
    return tuple(r[k] for k in KEYS)


def _fresh(hists, o):
    with core.Batch(hists, core.make_model(N.MODEL_MUTEX, 0), o) as b:
        return [_key(r) for r in b.run().results()]


@pytest.mark.parametrize("lanes", [8, 64])
def test_fresh_mutex_inputs_are_answered_as_their_own_batch_would(native, oracle, lanes):
    """:acquire / :release and an all-nil value column through the 12 B/op wire format: a batch reloaded twice with other histories
    of other lengths and counts answers each input as a batch created from it; what it cannot take is refused by name."""
    o = opts(algorithm=N.ALG_COMPETITION, want_witness=False, lanes_per_history=lanes, search_width=0 if lanes == 8 else 4)
    first = _mutex_set(1000, 96)
    with core.Batch(first, core.make_model(N.MODEL_MUTEX, 0), o) as b:
        base = [_key(r) for r in b.run().results()]
        assert base == _fresh(first, o)
        n_bad = 0
        for rnd in range(2):
            nxt = _mutex_set(2000 + 500 * rnd, 90 - 13 * rnd, n_ops=200 + 150 * rnd)
            b.reload(nxt)
            res = b.run().results()
            assert len(res) == len(nxt) and [_key(r) for r in res] == _fresh(nxt, o), rnd
            info = b.input_info()
            assert info["n_hist"] == len(nxt) and info["pending"] == 0 and info["inputs_consumed"] == rnd + 1
            assert info["bytes_copied"] == 12 * sum(len(h) for h in nxt)
            for i in (0, 1, 5, len(nxt) - 1):
                ref = oracle.check(nxt[i].as_dict(), MH.MUTEX, "window", max_steps=MH.MAX_STEPS, want_witness=False)
                assert ref["valid"] != -1
                assert res[i]["valid"] == ref["valid"] and (ref["valid"] == 1 or res[i]["fail_op"] == ref["fail_op"]), (rnd, i)
                n_bad += ref["valid"] == 0
        assert n_bad >= 2
        b.reload(_mutex_set(3000, 16, info=0.05, bad_every=0))          # a crashed call into a batch created without any
        with pytest.raises(N.TbcError) as e:
            b.run()
        assert e.value.status == N.ERR_UNSUPPORTED and "crashed" in e.value.detail
        b.reload(first)                                                 # ... and the batch still answers its first input
        assert [_key(r) for r in b.run().results()] == base


def test_fresh_mutex_inputs_with_crashed_calls_and_the_table_refused(native, oracle):
    """The mask form (a bit per crashed call): a mutex batch created from histories with crashed calls takes others.  A table batch
    takes no fresh inputs and says so."""
    o = opts(algorithm=N.ALG_COMPETITION, want_witness=False, lanes_per_history=8, count_form=False, max_steps=200000)
    first = _mutex_set(4000, 24, n_ops=200, info=0.02, bad_every=0)
    nxt = _mutex_set(4100, 20, n_ops=250, info=0.03, bad_every=0)
    assert sum(MH.n_crashed(h) for h in first) > 0 and sum(MH.n_crashed(h) for h in nxt) > 0          # both sets hold crashed calls
    with core.Batch(first, core.make_model(N.MODEL_MUTEX, 0), o) as b:
        b.run()
        b.reload(nxt)
        got = [_key(r) for r in b.run().results()]
        assert got == _fresh(nxt, o)
        assert all(g[0] != N.UNKNOWN for g in got)
    cases = MH.references(oracle, ["table-1", "table-1-bad"])
    with core.Batch([c.ops for c in cases], cases[0].native, opts(algorithm=N.ALG_COMPETITION, want_witness=False, search_width=4)) as b:
        with pytest.raises(N.TbcError) as e:
            b.map_input(0)
        assert e.value.status == N.ERR_UNSUPPORTED


# ---- what ships: nothing pinned (the count form by default, the library's own list order)
@pytest.fixture
def shipped_defaults():
    old = core.DEFAULT_COUNT_FORM, core.DEFAULT_LIST_ORDER
    core.DEFAULT_COUNT_FORM, core.DEFAULT_LIST_ORDER = True, 0
    yield
    core.DEFAULT_COUNT_FORM, core.DEFAULT_LIST_ORDER = old


@pytest.mark.parametrize("algorithm,witness", [(N.ALG_COMPETITION, False), (N.ALG_COMPETITION, True), (N.ALG_WGL, True), (N.ALG_LINEAR, False)])
@pytest.mark.parametrize("group", GROUPS)
def test_under_the_shipped_defaults(native, oracle, shipped_defaults, group, algorithm, witness):
    """tbc_opts all zero but the algorithm -- the list order "a :write as if it completed 24 ranks later" over histories without a
    :write, the sweep for a handful of histories: verdict and failing op are the sequential oracle's, every witness is a legal run."""
    cases = MH.references(oracle, names_of(group))
    if algorithm in (N.ALG_WGL, N.ALG_LINEAR):
        # (the published forms keep a mask bit per crashed call: an invalid history with crashed calls is exponential for them --
        # tests/test_shipped_defaults_gpu.py; crash-free or under 250 ops)
        cases = [c for c in cases if c.ref["valid"] == 1 or c.crashed == 0 or len(c.ops) < 250]
    assert {c.ref["valid"] for c in cases} == {0, 1}
    o = core.make_opts(time_limit_ms=20000, algorithm=algorithm, want_witness=witness)

    def same(got, c, tag):
        assert got["valid"] == c.ref["valid"], (tag, c.name, got["valid"], got["cause"])
        if c.ref["valid"] == 0:
            assert got["fail_op"] == c.ref["fail_op"], (tag, c.name)
        elif got["witness"] is not None:
            replay(c, got, (tag, c.name))
        assert not (witness and c.ref["valid"] == 1 and got["witness"] is None), (tag, c.name)

    for c in cases:
        same(core.check_ops(c.ops, c.native, o), c, "single")
    with core.Batch([c.ops for c in cases], cases[0].native, o) as b:
        for c, got in zip(cases, b.run().results()):
            same(got, c, "batch")


# ---- the knossos surface
@pytest.mark.parametrize("which", ["mutex", "table"])
def test_knossos_surface_over_generated_histories(native, oracle, which):
    """wgl / linear / competition analysis over M.mutex() and the no-overdraft M.Bank: :valid? and the failing op's :index are the
    oracle's; an invalid verdict's :configs carry models of the right kind -- the bank's decoded from the memo table's state."""
    for bad in (False, True):
        if which == "mutex":
            model, hist = M.mutex(), MH.mutex_history(300, 8, 71, busy=0.5, corrupt=MH.MUTEX_CORRUPT if bad else None)
            enc, om = MH.encode_mutex(hist)
        else:
            model, hist = MH.table_model(), MH.table_history(300, 8, 72, busy=0.15, corrupt=bad)
            enc, om = MH.encode_table(hist)
        assert 200 <= len(enc.ops) <= 400
        exp = oracle.check(enc.ops.as_dict(), om, "window", max_steps=MH.MAX_STEPS)
        assert exp["valid"] == (0 if bad else 1)
        total, rows = oracle.last_configs("window") if bad else (0, [])
        for name, analysis in (("wgl", wgl.analysis), ("linear", linear.analysis), ("competition", competition.analysis)):
            a = analysis(model, hist)
            assert a["valid?"] is (not bad), name
            if not bad:
                continue
            assert a["op"]["index"] == enc.op_completion(exp["fail_op"])["index"] and a["op"]["type"] == "ok", name
            assert a["configs"] and 0 < total <= 4096, name
            assert all(isinstance(c["model"], M.Mutex if which == "mutex" else M.Bank) for c in a["configs"]), name
            # the configs stuck in front of the failing completion are a property of the history (these models have no dominance
            # rules): every engine reports some of the oracle's, the sequential one the first ten in the oracle's order
            stuck = {int(r[0]) for r in rows}
            decode = (lambda s: M.Mutex(bool(s))) if which == "mutex" else (lambda s: enc.table_info["states"][s])
            assert all(c["model"] in {decode(s) for s in stuck} for c in a["configs"]), name
            if name == "wgl":
                assert len(a["configs"]) == min(total, 10)
                assert [c["model"] for c in a["configs"]] == [decode(int(r[0])) for r in rows[:10]], name

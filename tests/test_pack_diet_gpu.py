"""The pack's two counting steps ON THE DEVICE (csrc/pack_one_impl.h phase 4: the same-process count by ballots; csrc/open_walk_impl.h
phase A2: a candidate's place from a bitmap of the keys), through core.Batch at the small shapes of tests/test_pack_diet_emu.py, against
the oracle's schedule: a record in the wrong place of its process's list or a list in the wrong order changes the counters, the witness
or the verdict."""
import numpy as np
import pytest

from jepsen_tigerbeetle_amd import _native as N, columns, core, synth

pytestmark = pytest.mark.gpu

CAS = {"kind": 1, "init": N.NIL}
STEPS = 3000            # the crowded histories are not searched to the end: both sides stop after the round that passes this many probes


def _h(n, p, busy, info=0.0, seed=1):
    return columns.pair_events(synth.register_events(n_ops=n, n_procs=p, seed=seed, busy=busy, info=info))


def _small_shapes():
    """2 - 3 processes x 200 ops (many ops of one process in a 64-op chunk, a last chunk of 8), a 1-op history, all 64 slots in use,
    and chunks of the walk with at most 64, 65 - 128 and more than 128 candidates, crashed calls among them"""
    hs = [_h(200, 2, 1.0, seed=1), _h(200, 3, 0.7, seed=2), _h(200, 3, 1.0, seed=3), _h(1, 1, 0.5, seed=4), _h(1000, 64, 0.1, seed=1),
          _h(300, 6, 0.5, seed=1), _h(400, 40, 1.0, info=0.01, seed=2), _h(400, 58, 1.0, info=0.01, seed=3), _h(400, 64, 0.9, seed=4)]
    assert all(h.n_process <= 64 for h in hs)
    assert {0, 31, 32, 63} <= set(np.asarray(hs[4].process).tolist())
    return hs


_EXPECT = {}


def _expect(oracle, hists, order):
    if order not in _EXPECT:
        _EXPECT[order] = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False,
                                            list_order=oracle.ORACLE_LIST_ORDER[order], max_probes=STEPS) for h in hists]
    return _EXPECT[order]


# (what is asked, csrc PackOpenArgs.list_order: 0 slot order, 1 completion order, 2 the writes last, 16 + W)
@pytest.mark.parametrize("asked,order", [(N.ORDER_SLOT, 0), (N.ORDER_COMPLETION, 1), (N.ORDER_WRITES_LAST, 2), (16, 16), (N.ORDER_DEFAULT, 16 + 24)])
def test_small_shapes_through_the_narrow_kernels_pack(native, oracle, asked, order):
    """pack_wg64_kernel and open_walk_fronts_kernel<8> in every list order; run twice, the same both times"""
    hists = _small_shapes()
    n1 = len(hists)
    exp = _expect(oracle, hists, order)
    done = [len(h) > 1 for h in hists]                             # (the 1-op history, a read of nil, is decided at the root: the library counts no config for it)
    assert done.count(False) == 1
    opts = core.make_opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8, want_witness=False, list_order=asked, count_form=False, max_steps=STEPS)
    with core.Batch(hists * 10, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:      # (enough histories that no level sweep runs beside the search)
        assert b.lanes_per_history() == 8
        res = b.run().results()
        again = b.run().results()
    for i, got in enumerate(res):
        e = exp[i % n1]
        assert got["valid"] == e["valid"] and (e["valid"] != -1 or got["cause"] == N.CAUSE_STEP_LIMIT), (i, got["valid"], e["valid"], got["cause"])
        if done[i % n1]:
            assert (got["probes"], got["visited"]) == (e["probes"], e["visited"]), i
        if e["valid"] == 0:
            assert got["fail_op"] == e["fail_op"], i
        assert (again[i]["valid"], again[i]["probes"], again[i]["visited"]) == (got["valid"], got["probes"], got["visited"]), i


def test_130_processes_through_the_wide_kernels_pack(native, oracle):
    """pack_wg_kernel: slot numbers up to 129 (the eighth bit), few calls in flight so that the search stays small"""
    hists = [_h(2000, 130, 0.05, seed=s) for s in (1, 2)]
    assert all(h.n_process == 130 and int(np.asarray(h.process).max()) == 129 for h in hists)
    opts = core.make_opts(algorithm=N.ALG_COMPETITION, search_width=4, want_witness=False, order_restarts=False, count_form=False, time_limit_ms=60000)
    with core.Batch(hists * 11, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        assert b.lanes_per_history() == 64
        res = b.run().results()
    for i, h in enumerate(hists):
        e = oracle.check_beam(h.as_dict(), CAS, 4, want_witness=False, max_probes=20_000_000)
        for got in res[i::len(hists)]:
            assert got["valid"] == e["valid"], (i, got["valid"], e["valid"], got["cause"])
            assert (got["probes"], got["visited"]) == (e["probes"], e["visited"]), i


def test_count_form_with_slotless_calls(native, oracle):
    """count form: a crashed call holds no slot -- the verdict and the failing op are the sequential search's"""
    hists = [_h(200, 3, 1.0, info=0.2, seed=1), _h(300, 16, 0.5, info=0.3, seed=2), _h(130, 4, 1.0, info=0.5, seed=3)]
    hists += [columns.pair_events(synth.register_events(n_ops=120, n_procs=8, seed=s, busy=0.5, info=0.1, corrupt=0.5)) for s in (4, 5)]
    assert all((np.asarray(h.ret_pos) == 0xFFFFFFFF).sum() > 10 for h in hists)
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, search_width=4, want_witness=False, count_form=True)
    with core.Batch(hists * 11, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        res = b.run().results()
    for i, h in enumerate(hists):
        e = oracle.check(h.as_dict(), CAS, "window")
        for got in res[i::len(hists)]:
            assert got["valid"] == e["valid"], (i, got["valid"], e["valid"], got["cause"])
            if e["valid"] == 0:
                assert got["fail_op"] == e["fail_op"], i


def test_sets_that_grow_from_the_pool_run_after_run_and_reloaded(native, oracle):
    """first visited sets of one entry per op: histories outgrow theirs inside the kernel and take larger ones from the growth pool -- of
    which a pass zeroes only what the last one was handed (csrc/pool_plan.h).  Three runs, the same histories reloaded, then reloaded
    in another order (other histories get the pool's first words): verdicts and counters are the oracle's every time."""
    small = [_h(300, 16, 0.5, seed=s) for s in range(8)]
    big = [columns.pair_events(synth.register_events(n_ops=2500, n_procs=16, seed=s, busy=0.25, corrupt=c)) for s in range(8) for c in (0.0, 0.4)]
    hists = small + big
    exp = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False) for h in hists]
    want = [(e["valid"], e["probes"], e["visited"], e["fail_op"] if e["valid"] == 0 else None) for e in exp]
    key = lambda r: (r["valid"], r["probes"], r["visited"], r["fail_op"] if r["valid"] == 0 else None)
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=1, want_witness=False)
    with core.Batch(hists, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        for run in range(3):
            res = b.run().results()
            assert [key(r) for r in res] == want, run
            assert max(r["table_slots"] for r in res) >= 4 * 4096, run          # (the sets did grow)
        b.reload(hists)
        assert [key(r) for r in b.run().results()] == want
        b.reload(hists[::-1])
        assert [key(r) for r in b.run().results()] == want[::-1]
        assert [key(r) for r in b.run().results()] == want[::-1]

"""The sparse form of the front walk's phase C ON THE DEVICE (csrc/open_walk_impl.h: membership by prefix-XOR of toggle events, entries and
twin masks per front, the producer distance from byte counters), through core.Batch at the small shapes of tests/test_walk_sparse_emu.py,
against the oracle's schedule: a call missing from or left too long in a front's list, a wrong twin mask, read row or lookahead record
changes the counters, the failing op or the verdict."""
import numpy as np
import pytest

from jepsen_tigerbeetle_amd import _native as N, core

import walk_sparse_shapes as shapes

pytestmark = pytest.mark.gpu

CAS = {"kind": 1, "init": N.NIL}
STEPS = 3000            # the crowded histories are not searched to the end: both sides stop after the round that passes this many probes

_HISTS = []
_EXPECT = {}


def _hists():
    if not _HISTS:
        rs = shapes.runs_shapes
        more = [h for h in rs.ragged() + rs.few_processes() + rs.all_busy() + [rs.planted()] if len(h) <= 700]
        _HISTS.extend((shapes.hand_built() + more)[:33])           # (three copies of each: under a hundred histories a batch)
        assert len(_HISTS) >= 25 and all(h.n_process <= 64 and len(h) <= 700 for h in _HISTS)
    return _HISTS


def _expect(oracle, order):
    if order not in _EXPECT:
        _EXPECT[order] = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False,
                                            list_order=oracle.ORACLE_LIST_ORDER[order], max_probes=STEPS) for h in _hists()]
    return _EXPECT[order]


def _compare(res, exp, hists):
    n1 = len(hists)
    for i, got in enumerate(res):
        e = exp[i % n1]
        assert got["valid"] == e["valid"] and (e["valid"] != -1 or got["cause"] == N.CAUSE_STEP_LIMIT), (i, got["valid"], e["valid"], got["cause"])
        if len(hists[i % n1]) > 1:                                 # (a 1-op history, a read of nil, is decided at the root: the library counts no config for it)
            assert (got["probes"], got["visited"]) == (e["probes"], e["visited"]), i
        if e["valid"] == 0:
            assert got["fail_op"] == e["fail_op"], i


# (what is asked, csrc PackOpenArgs.list_order: 0 slot order, 1 completion order, 16 + W)
@pytest.mark.parametrize("asked,order", [(N.ORDER_SLOT, 0), (N.ORDER_COMPLETION, 1), (16, 16), (N.ORDER_DEFAULT, 16 + 24)])
def test_small_shapes_through_the_sparse_form(native, oracle, asked, order):
    """pack_wg64_kernel and open_walk_fronts_kernel<8>, then the narrow search: a slot handed on at every front, a call open over three
    chunks, crashed producers, twelve calls open at once with shared effects, a cas v v with and without another producer, last chunks of 1
    and 63 fronts, 64 busy slots (more than 128 candidates a chunk)"""
    hists = _hists()
    exp = _expect(oracle, order)
    opts = core.make_opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8, want_witness=False, list_order=asked, count_form=False, max_steps=STEPS)
    with core.Batch(hists * 3, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:      # (enough histories that no level sweep runs beside the search)
        assert b.lanes_per_history() == 8
        res = b.run().results()
    _compare(res, exp, hists)


def test_values_up_to_30(native, oracle):
    """rows of 32 entries: open_walk_fronts_kernel<32>, which keeps the dense loop"""
    hists = [shapes.runs_shapes.gen(300, 24, 0.6, seed=s, n_values=31) for s in (4, 5)] + [shapes.handover(3, 100)]
    assert max(int(np.asarray(h.a).max()) for h in hists[:2]) == 30
    exp = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False,
                             list_order=oracle.ORACLE_LIST_ORDER[16 + 24], max_probes=STEPS) for h in hists]
    opts = core.make_opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8, want_witness=False, list_order=N.ORDER_DEFAULT, count_form=False, max_steps=STEPS)
    with core.Batch(hists * 30, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        assert b.lanes_per_history() == 8
        res = b.run().results()
    _compare(res, exp, hists)


def test_count_form_with_slotless_crashed_calls(native, oracle):
    """count form: the crashed calls hold no slot and are not among the walk's candidates, the live ones re-use slots -- verdict and failing
    op are the sequential search's"""
    hists = [shapes.runs_shapes.gen(300, 3, 1.0, info=0.2, seed=6), shapes.runs_shapes.gen(500, 16, 0.5, info=0.3, seed=7), shapes.crashed_producer()]
    assert all((np.asarray(h.ret_pos) == 0xFFFFFFFF).sum() >= 2 for h in hists)
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, search_width=4, want_witness=False, count_form=True)
    with core.Batch(hists * 11, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        res = b.run().results()
    for i, h in enumerate(hists):
        e = oracle.check(h.as_dict(), CAS, "window")
        for got in res[i::len(hists)]:
            assert got["valid"] == e["valid"], (i, got["valid"], e["valid"], got["cause"])
            if e["valid"] == 0:
                assert got["fail_op"] == e["fail_op"], i

"""The sparse form's list stores with lane = entry ON THE DEVICE (csrc/open_walk_impl.h, sparse_lists: a chunk's list entries taken 64 at a
time, whole lines a store), through core.Batch at the hand-built shapes of tests/test_walk_lines_emu.py plus three dozen generated histories
of at most 512 ops in one batch, against the oracle's schedule: an entry that takes the wrong front's call, a wrong rank within the front, a
twin mask from another front or an entry stored out of place changes the counters, the failing op or the verdict."""
import numpy as np
import pytest

from jepsen_tigerbeetle_amd import _native as N, core

import walk_lines_shapes as shapes

pytestmark = pytest.mark.gpu

CAS = {"kind": 1, "init": N.NIL}
STEPS = 3000            # the crowded histories are not searched to the end: both sides stop after the round that passes this many probes

_HISTS = []
_EXPECT = {}


def _hists():
    if not _HISTS:
        _HISTS.extend(shapes.hand_built() + shapes.generated(36))
        assert 40 <= len(_HISTS) <= 47 and all(h.n_process <= 64 and len(h) <= 512 for h in _HISTS)
    return _HISTS


def _expect(oracle, order):
    if order not in _EXPECT:
        _EXPECT[order] = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False,
                                            list_order=oracle.ORACLE_LIST_ORDER[order], max_probes=STEPS) for h in _hists()]
    return _EXPECT[order]


# (what is asked, csrc PackOpenArgs.list_order: 0 slot order, 1 completion order, 16 + W)
@pytest.mark.parametrize("asked,order", [(N.ORDER_SLOT, 0), (N.ORDER_COMPLETION, 1), (16, 16), (N.ORDER_DEFAULT, 16 + 24)])
def test_lists_stored_by_entry(native, oracle, asked, order):
    """pack_wg64_kernel and open_walk_fronts_kernel<8>, then the narrow search: chunks of 0, 1, 63, 64, 65, 127 and 128 entries, a front whose
    entries lie in two passes, a front that begins with a pass, empty fronts between full ones, a dense chunk between two sparse ones of a run,
    twelve calls open at once (places in the second set), last chunks of 1 and 63 fronts, and the generated histories"""
    hists = _hists()
    exp = _expect(oracle, order)
    opts = core.make_opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8, want_witness=False, list_order=asked, count_form=False, max_steps=STEPS)
    with core.Batch(hists * 3, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:      # (enough histories that no level sweep runs beside the search)
        assert b.lanes_per_history() == 8
        res = b.run().results()
    n1 = len(hists)
    for i, got in enumerate(res):
        e = exp[i % n1]
        assert got["valid"] == e["valid"] and (e["valid"] != -1 or got["cause"] == N.CAUSE_STEP_LIMIT), (i, got["valid"], e["valid"], got["cause"])
        assert (got["probes"], got["visited"]) == (e["probes"], e["visited"]), i
        if e["valid"] == 0:
            assert got["fail_op"] == e["fail_op"], i


def test_count_form_batch(native, oracle):
    """count form: the crashed calls hold no slot and are not among the walk's candidates, the live ones re-use slots -- verdict and failing
    op are the sequential search's"""
    gen = shapes.sparse_shapes.runs_shapes.gen
    hists = [gen(300, 3, 1.0, info=0.2, seed=16), gen(400, 16, 0.5, info=0.2, seed=18), shapes.sparse_shapes.crashed_producer(), shapes.counted_chunks()]
    assert all((np.asarray(h.ret_pos) == 0xFFFFFFFF).sum() >= 2 for h in hists[:3])
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, search_width=4, want_witness=False, count_form=True)
    with core.Batch(hists * 11, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        res = b.run().results()
    for i, h in enumerate(hists):
        e = oracle.check(h.as_dict(), CAS, "window")
        for got in res[i::len(hists)]:
            assert got["valid"] == e["valid"], (i, got["valid"], e["valid"], got["cause"])
            if e["valid"] == 0:
                assert got["fail_op"] == e["fail_op"], i

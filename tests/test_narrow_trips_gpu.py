"""K5n on the device at the shapes where its once-rare paths are routine (tests/test_narrow_trips_emu.py counts them on the CPU:
more than 16 and 24 viable children in a wavefront, a front advancing past its record's window, two lanes of a group wanting the
same empty entry, full buckets): 8 lanes per history through core.Batch in the shipped list order, first visited sets of 4 entries
and of 1 entry per op, with and without a witness -- verdict, failing op, witness and every counter against the oracle's schedule."""
import numpy as np
import pytest

from jepsen_tigerbeetle_amd import _native as N, columns, core, synth

pytestmark = pytest.mark.gpu

CAS = {"kind": 1, "init": N.NIL}


@pytest.fixture(scope="module")
def cases(oracle):
    """the histories and what the oracle says about each, once for every test here"""
    oracle.build()
    hists = [columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.5, seed=s)) for s in range(100, 116)]
    hists += synth.register_ops_many(range(7000, 7064), n_ops=1000, n_procs=64, busy=0.1)
    exp = [oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, list_order=16 + 24, want_witness=True) for h in hists]
    return hists, exp


@pytest.mark.parametrize("want_witness", [True, False])
@pytest.mark.parametrize("visited_per_op", [4, 1])
def test_narrow_kernel_at_the_shapes_that_take_every_path(native, cases, visited_per_op, want_witness):
    hists, exp = cases
    n1 = len(hists)
    # (the 80 histories eight times over: groups refill from the queue, and the batch is large enough that the search runs alone)
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=visited_per_op,
                          want_witness=want_witness, list_order=N.ORDER_DEFAULT, count_form=False)
    with core.Batch(hists * 8, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        assert (b.lanes_per_history(), b.search_width(), b.list_order()) == (8, 1, 16 + 24)
        res = b.run().results()
    assert len(res) == 8 * n1
    for k, got in enumerate(res):
        i, e = k % n1, exp[k % n1]
        assert got["valid"] == e["valid"] == 1, (k, got["valid"], got["cause"])
        assert (got["probes"], got["visited"], got["backtracks"], got["max_depth"]) == (e["probes"], e["visited"], e["expanded"], e["max_stack"]), (k, i)
        assert got["final_state"] == e["final_state"], k
        if want_witness and k < n1:
            assert got["witness"] is not None and np.array_equal(got["witness"], e["witness"]), k


def test_planted_bad_reads_fail_at_the_oracles_op(native, oracle):
    """the same shape with a bad read planted: INVALID at the oracle's op after the oracle's number of probes (every bucket chain walked to its end)"""
    hists = []
    for s in range(200, 216):
        h = columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.5, seed=s, corrupt=0.5, n_values=4))
        h.a[h.a == 4 + 7] = 4                 # (the planted value stays inside the domain of the compact front records: 0..4)
        hists.append(h)
    opts = core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, lanes_per_history=8, visited_per_op=4, want_witness=False,
                          list_order=N.ORDER_DEFAULT, count_form=False)
    with core.Batch(hists * 16, core.make_model(N.MODEL_CAS_REGISTER, N.NIL), opts) as b:
        res = b.run().results()
    n_bad = 0
    for i, h in enumerate(hists):
        e = oracle.check_beam(h.as_dict(), CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, list_order=16 + 24, want_witness=False)
        for k in (i, i + 16 * 7, i + 16 * 15):
            got = res[k]
            assert got["valid"] == e["valid"], (k, got["valid"], e["valid"], got["cause"])
            assert (got["probes"], got["visited"], got["backtracks"], got["max_depth"]) == (e["probes"], e["visited"], e["expanded"], e["max_stack"]), k
            if e["valid"] == 0:
                assert got["fail_op"] == e["fail_op"], k
        n_bad += e["valid"] == 0
    assert n_bad >= 4

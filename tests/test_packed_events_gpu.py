"""tbc_pair_packed_batch on the MI355X: the shapes of tests/packed_events_shapes.py through the entry point -- the packed reader of
csrc/pair_kernels.h -- every array bit for bit what tbc_pair_events gives over what the words decode to (descriptors, status, bad row,
wire word, positions, and the columns), what is copied in (8 B a row), and the capacity rule at exactly the need and at one below."""
import numpy as np
import pytest

import packed_events_shapes as P
import pair_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns

pytestmark = pytest.mark.gpu

CASES = sorted(P.cases())


def run(evs, ops_cap=None):
    ev_off, words, process = P.concat_packed(evs)
    return columns.pair_events_batch_raw(ev_off, (words, process), ops_cap=ops_cap, word=True)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_tbc_pair_events_over_the_decoded_events(native, name):
    evs = P.cases()[name]
    st, got = run(evs)
    N.check_status(st)
    S.assert_same(got, P.packed_reference(name, evs), name)
    assert got["bytes_in"] == 8 * sum(len(e) for e in evs) + 8 * (len(evs) + 1)


def test_random_histories_in_one_call(native):
    evs = S.random_batch()
    st, got = run(evs)
    N.check_status(st)
    S.assert_same(got, P.packed_reference("random", evs), "random")
    assert got["ns_device"] > 0 and got["bytes_in"] == 8 * sum(len(e) for e in evs) + 8 * (len(evs) + 1)


def test_capacity_exact_and_one_below(native):
    evs = P.cases()["bad_among_good"]
    want = P.packed_reference("bad_among_good", evs)
    T = want["n_ops"]
    guard = lambda n, dt: np.full(n, 0xA5, dt)
    ev_off, words, process = P.concat_packed(evs)
    # one below: refused with the count, nothing written; at the need: the ops, and the words behind them as they were
    for cap, status in ((T - 1, N.ERR_INVALID_ARG), (T, 0)):
        st, got = columns.pair_events_batch_raw(ev_off, (words, process), ops_cap=cap, word=True, alloc=lambda n, dt: guard(T + 7, dt))
        assert st == status
        if status:
            assert f"{T} ops survive" in native.lib().tbc_last_error().decode()
        for k in ("f", "a", "b", "process", "inv_pos", "ret_pos", "word"):
            n = T if status == 0 else 0
            assert np.array_equal(got[k][:n], want[k][:n]) and (got[k][n:] == guard(1, got[k].dtype)[0]).all(), (cap, k)

"""tbc_pair_keyed_events on the MI355X: every shape of tests/keyed_events_shapes.py through the entry point, in both forms of the
events (the five columns; the packed word), every array bit for bit what columns.split_events in numpy followed by tbc_pair_events
key by key gives -- keys, ev_off, row_of, the descriptors, the six op columns, the wire word, status and bad row; keys_cap exact and
one below; the split alone (out == NULL); row_of wanted and not wanted; the Python surface."""
import numpy as np
import pytest

import keyed_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns

pytestmark = pytest.mark.gpu

CASES = sorted(S.cases())


@pytest.mark.parametrize("name", CASES)
def test_device_equals_split_events_and_tbc_pair_events(native, name):
    for i, (ev, key) in enumerate(S.cases()[name]):
        for packed, word in S.forms(name):
            st, got = columns.pair_keyed_events_raw(S.packed(ev) if packed else ev, key, word=word)
            N.check_status(st)
            S.assert_same(got, S.reference(name, i, ev, key, word, packed), (name, i, packed, word))
            assert got["bytes_in"] == (12 if packed else 18) * len(key)


def test_keys_cap_exact_and_one_below(native):
    ev, key = S.cases()["refusal_per_key"][0]
    want = S.reference("refusal_per_key", 0, ev, key, False)
    nk = want["n_keys"]
    st, got = columns.pair_keyed_events_raw(ev, key, keys_cap=nk)
    N.check_status(st)
    S.assert_same(got, want, "keys_cap = n_keys")
    assert got["ns_device"] > 0
    st, got = columns.pair_keyed_events_raw(ev, key, keys_cap=nk - 1)
    assert st == N.ERR_INVALID_ARG and f"{nk} distinct keys" in native.lib().tbc_last_error().decode()
    assert got["n_keys"] == 0 and not got["row_of"].any() and got["n_ops"] == 0 and not got["inv_pos"].any()


def test_split_only_and_row_of_not_wanted(native):
    ev, key = S.cases()["chunk_and_tile_edges"][0]
    want = S.reference("chunk_and_tile_edges", 0, ev, key, False)
    st, got = columns.pair_keyed_events_raw(ev, key, pair=False)
    N.check_status(st)
    S.assert_same(got, want, "split only", paired=False)
    st, got = columns.pair_keyed_events_raw(ev, key, row_of=False, columns=False)
    N.check_status(st)
    assert "row_of" not in got and "f" not in got
    S.assert_same(got, {k: v for k, v in want.items() if k not in ("f", "a", "b", "process")}, "no row_of", row_of=False)
    st, got = columns.pair_keyed_events_raw(S.packed(ev), key, pair=False, row_of=False)
    N.check_status(st)
    S.assert_same(got, want, "split only, packed, no row_of", row_of=False, paired=False)


def test_python_surface(native):
    ev, key = S.cases()["refusal_per_key"][0]
    keys, ops, status, bad_row, row_of = columns.pair_keyed_events(ev, key)
    want_keys, ev_off, want_rows = columns.split_events(ev, key)
    assert list(keys) == list(want_keys) == [1, 2, 3, 4, 5, 6, 7] and np.array_equal(row_of, want_rows)
    assert [o is None for o in ops] == [False, True, False, True, False, True, False]
    assert list(status[[1, 3, 5]]) == [N.ERR_BAD_HISTORY, N.ERR_UNSUPPORTED, N.ERR_BAD_HISTORY] and list(bad_row[[1, 5]]) == [20, 0]
    for h, o in enumerate(ops):
        if o is not None:
            want = columns.pair_events(columns.take_events(ev, want_rows[int(ev_off[h]):int(ev_off[h + 1])]))
            assert (o.n_events, o.n_process) == (want.n_events, want.n_process)
            for k in ("f", "a", "b", "process", "inv_pos", "ret_pos"):
                assert np.array_equal(getattr(o, k), getattr(want, k)), (h, k)

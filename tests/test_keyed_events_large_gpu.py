"""tbc_pair_keyed_events on the MI355X past the sizes at which its kernels change behaviour under the library's own launcher
(keyed_events_shapes.large_case): more than 2^20 rows -- sp_top_kernel takes a second step of 256 block sums, and the row kernels
(insert, rid, gather) stride over their grid of 4,096 workgroups --, with two and with three passes of the sort, several rows a key
through three passes, and more than 8,192 tiles, where the tile kernels (first rows, ids, histogram, scatter) stride.  The split
alone in both forms of the events, keys, ev_off and row_of bit for bit against columns.split_events; ONE paired call, which is what
holds the gather's strided writes of the events to account, through every array of the pairing; keys_cap exact and one below with
a count above 65,536 read back from the first scan.  The call reports bytes_in through `out`, which the split alone does not have:
the paired calls hold it, 12 B a row packed and 18 B in columns.  (The two small shapes of this change, probe_run_wraps and
many_rows_over_passes, are in cases(): tests/test_keyed_events_gpu.py runs them.)  The batch entrance runs the same two launch
sequences and is not repeated here."""
import numpy as np
import pytest

import keyed_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("packed", [False, True], ids=["columns", "packed"])
@pytest.mark.parametrize("name", S.LARGE_GPU_CASES)
def test_split_past_the_thresholds(native, name, packed):
    ev, key = S.large_case(name)
    st, got = columns.pair_keyed_events_raw(S.packed(ev) if packed else ev, key, pair=False)
    N.check_status(st)
    S.assert_same(got, S.large_reference(name), (name, packed), paired=False)


@pytest.mark.parametrize("packed", [False, True], ids=["columns", "packed"])
def test_paired_past_2_to_the_20_rows(native, packed):
    """the events themselves through the gather's stride (g_word / the four columns, g_process): every array of the pairing against
    tbc_pair_events key by key, the packed form with the wire word"""
    name = "top_scan_second_step"
    ev, key = S.large_case(name)
    st, got = columns.pair_keyed_events_raw(S.packed(ev) if packed else ev, key, word=packed)
    N.check_status(st)
    S.assert_same(got, S.reference(name, 0, ev, key, packed, packed), (name, "paired", packed))
    assert got["bytes_in"] == (12 if packed else 18) * len(key)


def test_keys_cap_exact_and_one_below_above_65536_keys(native):
    """the refusal is decided before the sort, on the first scan's total: 70,000, read back"""
    name = "top_scan_three_passes"
    ev, key = S.large_case(name)
    want = S.large_reference(name)
    nk = want["n_keys"]
    assert nk == 70000
    st, got = columns.pair_keyed_events_raw(ev, key, keys_cap=nk, pair=False)
    N.check_status(st)
    S.assert_same(got, want, "keys_cap = n_keys", paired=False)
    st, got = columns.pair_keyed_events_raw(ev, key, keys_cap=nk - 1, pair=False)
    assert st == N.ERR_INVALID_ARG and f"{nk} distinct keys, keys_cap is {nk - 1}" in native.lib().tbc_last_error().decode()
    assert got["n_keys"] == 0 and not got["row_of"].any() and not got["ev_off"].any()

"""tbc_perf_series on the MI355X against the host statement of jepsen/perf.py, exactly: the raw arrays and the summary through the C
entry point, and the four series sets through both routes of `series` (latencies are integers until the host divides, and both routes
divide the same integers).  The shapes (tests/perf_histories.py shape_cases) are the smallest at which each kernel can go wrong:
  ops        0, 1 (a lone unmatched invocation), 2, 63 / 64 / 65, 255 / 256 / 257, 513
  cells      1, 2, 3, 20, 64, 65, 100, 101 latencies, every n in 1..130 once, one cell of more than the LDS tile (the radix select),
             ties throughout, latency 0, latencies above 2^32 ns beside small ones
  times      t_max and op times at k 10^9 - 1, k 10^9, k 10^9 + 5 10^8 - 1 / + 0 / + 1 (both values of n_plot), a pair across buckets,
             empty buckets to fill forward, ops in the unplotted last bucket, times that are not monotone, t_max by the nemesis alone
  classes    1 f, 9 f's, an f with only :fail, one with only unmatched invocations, :info, a process number reused after :info, a
             completion without an invocation
  open scan  one class over several chunks, two classes interleaved op by op, a count that is back to 0 on a chunk's edge
plus one seeded random history of about 20k ops.  Every reference is computed once (module fixture), which first asserts that each
case has the shape it is named for (perf_histories.references)."""
import numpy as np
import pytest

import perf_histories as G
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import perf as PF

pytestmark = pytest.mark.gpu

CASES = G.shape_cases()


@pytest.fixture(scope="module")
def refs(native):
    return G.references(CASES)


@pytest.fixture(scope="module")
def big():
    h = G.random_history(2024, 20_000, workers=64, fs=("read", "write", "cas", "add"), gap=1_500_000, info=0.03, fail=0.05, jitter=400_000_000)
    return h, G.expected(h)


def device_equals_host(h, want, n_ops, max_cell, ctx):
    cols = PF.PerfColumns(h)
    got = PF.check_native(cols)
    s = got["summary"]
    print(ctx, "ops", s["n_ops"], "largest cell", s["max_cell"], "ns_device", s["ns_device"])
    assert s["n_ops"] == n_ops == len(cols) and s["max_cell"] == max_cell           # what the case put on the device
    G.assert_same(got, want, ctx)
    assert s["bytes_in"] >= 19 * len(cols)                                            # time 8, process 4, type 1, f 2, the partner 4
    assert PF.series_from_device(h, cols, got) == PF.series_host(h), ctx


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_arrays_equal_host_statement(refs, case):
    want = refs[case["name"]]
    device_equals_host(case["history"], want, case["n_ops"], want["summary"]["max_cell"] if case["max_cell"] is None else case["max_cell"], case["name"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_both_routes_give_the_same_series(native, case):
    h = case["history"]
    assert PF.series(h, device_route=True) == PF.series(h, device_route=False), case["name"]


def test_random_history_of_20k_ops(native, big):
    h, want = big
    assert len(h) == 20_000 and want["summary"]["n_f"] == 4 and want["summary"]["max_cell"] > 64 and (want["op_latency"][want["op_latency"] != G.INT64_MIN] < 0).any()
    device_equals_host(h, want, 20_000, want["summary"]["max_cell"], "random 20k")
    assert PF.series(h, device_route=True) == PF.series(h, device_route=False)


def test_the_composed_checker_on_the_device(native, big):
    h, _ = big
    want = {"latency-graph": {"valid?": True}, "rate-graph": {"valid?": True}, "open-ops-graph": {"valid?": True}, "valid?": True}
    assert PF.perf({"device_route": True}).check({}, h, {}) == want and PF.DEVICE_ROUTE_DEFAULT is True and PF.perf().check({}, h, {}) == want


def test_a_cell_of_the_tile_and_one_more(native):
    """the threshold between the LDS sort and the radix select: cells of exactly TBC_PERF_SELECT_TILE and TBC_PERF_SELECT_TILE + 1"""
    T = N.PERF_SELECT_TILE
    h = G.cells_history((T, T + 1, T - 1), lambda k, i: ((i * 2654435761) % 1000003) * 977 + 4 * G.S)
    want = G.expected(h)
    assert [int(x) for x in want["q_count"][0][:3]] == [T, T + 1, T - 1]
    device_equals_host(h, want, len(h), T + 1, "tile edge")

"""tbc_ledger_snapshots on the MI355X against snapshots_numpy of jepsen/ledger.py, exactly: every output array and every summary field
through the C entry point -- n_checked, n_partial and n_candidates among them: on a valid history every count is 0, so those are what
tells a working kernel from an empty one, and a filter that over-flags fails on n_candidates --, the result map through
snapshots_result_map, the composed member through test(snapshots=True).  The shape cases (tests/ledger_snapshot_histories.py
shape_cases) are the smallest at which a kernel can go wrong: 0, 1, 2 equal and 2 skewed reads; 1 account (skew between its credits and
its debits), 8, 33 (more counters than lanes) and 1,025 accounts (past the accounts' table in LDS and any chunk of counters); 63, 64, 65
and 127, 128, 129 reads (64 reads are one step of a wavefront in the sort, one chunk of the scan and one tile of the pair kernel), with
a skewed pair at either end of the sorted order and without; 255, 256, 257 candidates (a block of the pair kernel is 256); 16,383,
16,384 and 16,385 reads of one account -- past 16,384 a chunk of the sort is two wavefronts' worth (the sort has 256 chunks at most, so
its carry has ONE level at every size) and the scan's carry over its chunks takes a second step of 256; sums that differ only in their
lowest byte, only in their highest and in sign, and in every byte; equal sums with different vectors; 200 identical reads; an
antichain of 300; one outlier skewed with all others; a complete read skewed only with a partial one (the atomic path onto a read that
is no candidate); reads that lack an account, hold a nil micro-op or a foreign id; partial reads only; reads of 300 micro-ops with
foreign ids; negative counters, values near 2^62 and at the ends of int64; a planted fork, a torn read, and the realtime plants, which
are valid here.  Each case has the `counts` it was built for.  References are computed once."""
import ctypes as C

import numpy as np
import pytest

import ledger_realtime_histories as G
import ledger_snapshot_histories as S
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L

pytestmark = pytest.mark.gpu

CASES = S.shape_cases()
ARRAYS = ("count", "first", "key", "flags")


def assert_same(got, want, tag):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")} == want["summary"], tag


def device(history, opts):
    cols = L.LedgerColumns(history)
    return cols, L.check_snapshots_native(cols, opts["accounts"])


@pytest.fixture(scope="module")
def refs(native):
    return {c["name"]: L.snapshots_numpy(c["history"], c["opts"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_numpy_statement(refs, case):
    want = refs[case["name"]]
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert (want["summary"]["skewed"]["count"] if k == "skewed" else want["summary"][k]) == v, (case["name"], k)
    cols, got = device(case["history"], case["opts"])
    assert_same(got, want, case["name"])
    s = got["summary"]
    assert s["n_checked"] == int(want["summary"]["n_checked"]) and (s["n_checked"] > 0 or s["read_count"] == 0)
    # only the reads' micro-ops are copied, 25 bytes each: transfers' and lookups' are not
    rd = (cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ)
    n_read_mops = int((cols.mop_off[1:][rd] - cols.mop_off[:-1][rd]).sum())
    assert 25 * n_read_mops <= s["bytes_in"] <= 25 * n_read_mops + 8 * len(cols.read_ops) + 12 * len(case["opts"]["accounts"]) + 16 * 256
    assert L.snapshots_result_map(case["history"], cols, got, case["opts"]["accounts"]) == L._snap_map(case["history"], cols.read_ops, want, case["opts"]["accounts"])


def test_random_vectors_with_partial_reads(native):
    import random
    rng = random.Random(23)
    for trial in range(10):
        accounts = rng.sample(range(1, 200), rng.choice((1, 2, 5, 17, 40)))
        h, o = S.reads_ledger(accounts, S.random_rows(rng, accounts, rng.randint(50, 600)), transfers_first=trial % 3)
        want = L.snapshots_numpy(h, o)
        assert_same(device(h, o)[1], want, trial)
        assert want["summary"]["n_partial"] > 0 and want["summary"]["n_pairs"] > 0


def test_random_concurrent_ledgers_valid_forked_and_torn(native):
    for seed, plant in enumerate([(), ("stale",), ("future",), ("regressed",)]):
        h, o, _ = G.concurrent_ledger(100 + seed, workers=8, ops=700, plant=plant)
        cols, got = device(h, o)
        assert_same(got, L.snapshots_numpy(h, o), plant)
        s = got["summary"]
        assert s["valid"] == 1 and s["n_candidates"] == 0 and s["n_partial"] == 0 and s["n_checked"] == 8 * s["read_count"] > 0
        assert L.snapshots_result_map(h, cols, got, o["accounts"]) == L.SnapshotOrder(o).check(o, h)
    h, o, planted = S.forked_ledger(110, forks=3, workers=8, ops=700)
    cols, got = device(h, o)
    assert_same(got, L.snapshots_numpy(h, o), "fork")
    assert got["summary"]["n_pairs"] == 3 and got["summary"]["n_candidates"] == 6
    for r, r2 in zip(planted["R"], planted["R2"]):
        assert got["first"][list(cols.read_ops).index(r)] == list(cols.read_ops).index(r2)
    assert L.snapshots_result_map(h, cols, got, o["accounts"]) == L.SnapshotOrder(o).check(o, h)
    h, o, r = S.torn_ledger(111, workers=8, ops=400)
    cols, got = device(h, o)
    assert_same(got, L.snapshots_numpy(h, o), "torn")
    assert got["count"][list(cols.read_ops).index(r)] > 0


def test_composed_member_device_route_equals_host_route(native):
    h, o, _ = S.forked_ledger(7, workers=5, ops=200)
    dev = L.test(o, realtime=True, snapshots=True, device_route=True)["checker"].check(o, h)
    host = L.test(o, realtime=True, snapshots=True, device_route=False)["checker"].check(o, h)
    assert dev == host
    assert dev["snapshots"]["valid?"] is False and dev["valid?"] is False
    assert all(dev[k]["valid?"] is True for k in ("SI", "lookup-transfers", "realtime"))       # the fork passes every existing member that judges reads
    h2, o2, _ = G.concurrent_ledger(7, workers=5, ops=200)
    res = L.test(o2, snapshots=True)["checker"].check(o2, h2)["snapshots"]
    assert res == L.SnapshotOrder(o2).check(o2, h2) and res["valid?"] is True and res["exact?"] is True
    assert "snapshots" not in L.test(o2)["checker"].check(o2, h2)


def test_no_accounts_at_all(native):
    """what only a direct caller of the C entry can ask: no account, so no counter: every read is complete and nothing is skewed"""
    h, o, _ = G.concurrent_ledger(5, ops=40)
    cols = L.LedgerColumns(h)
    got = L.check_snapshots_native(cols, [])
    assert_same(got, L.snapshots_dense_numpy(*L._snap_dense(cols, [])), "no accounts")
    assert got["summary"]["n_checked"] == 0 and got["summary"]["read_count"] == len(cols.read_ops) > 0


def test_invalid_input_is_refused_with_the_named_message(native):
    h, o, _ = G.concurrent_ledger(3, ops=30)

    def refused(change, needle):
        s, keep = L.ledger_snap_in(L.LedgerColumns(h), o["accounts"])              # (fresh columns: `change` writes into them)
        change(s, keep)
        out = N.LedgerSnapOut()
        assert N.lib().tbc_ledger_snapshots(C.byref(s), C.byref(out)) == N.ERR_INVALID_ARG
        msg = N.lib().tbc_last_error().decode()
        assert msg.startswith("tbc_ledger_snapshots") and needle in msg, msg

    refused(lambda s, k: setattr(s, "mop_off", None), "null argument (mop_off)")
    refused(lambda s, k: k["type"].__setitem__(4, 9), "op 4 (index")
    refused(lambda s, k: k["accounts"].__setitem__(1, 1), "account 1 is listed twice")
    refused(lambda s, k: k["index"].__setitem__(5, int(k["index"][4])), "strictly ascending")
    assert N.lib().tbc_ledger_snapshots(None, None) == N.ERR_INVALID_ARG


def test_magnitudes_that_reach_2_to_the_63_are_unsupported(native):
    h, o = S.reads_ledger([1, 2], S.chain_rows([1, 2], 70))
    for values in ((2 ** 62, 2 ** 62), (-(2 ** 63), 0)):
        cols = L.LedgerColumns(h)
        m = int(cols.mop_off[np.flatnonzero((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ))[66]])
        cols.mop_a[m], cols.mop_b[m] = values
        s, keep = L.ledger_snap_in(cols, o["accounts"])
        out = N.LedgerSnapOut()
        flags = np.full(70, 77, np.uint8)
        out.snap_flags = flags.ctypes.data_as(C.POINTER(C.c_uint8))
        assert N.lib().tbc_ledger_snapshots(C.byref(s), C.byref(out)) == N.ERR_UNSUPPORTED
        assert "2^63" in N.lib().tbc_last_error().decode() and out.summary.bad_values == 1
        assert (flags == 77).all()                                             # no results
        with pytest.raises(ValueError, match="2\\^63"):
            L.check_snapshots_native(cols, o["accounts"])
    cols = L.LedgerColumns(h)                                                  # one below: taken
    m = int(cols.mop_off[np.flatnonzero((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ))[66]])
    cols.mop_a[m], cols.mop_b[m] = 2 ** 62, 2 ** 62 - 3
    cols.mop_a[m + 1], cols.mop_b[m + 1] = 1, 1
    got = L.check_snapshots_native(cols, o["accounts"])
    assert_same(got, L.snapshots_dense_numpy(*L._snap_dense(cols, o["accounts"])), "2^63 - 1")

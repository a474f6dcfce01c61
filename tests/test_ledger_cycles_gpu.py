"""tbc_ledger_cycles on the MI355X against cycles_numpy of jepsen/ledger.py, exactly: both output arrays and every summary field through
the C entry point, closure_rounds included, and against cycles_host (the explicit graph and Tarjan) where a history has 64 reads at
most; the result map through cycles_result_map, the composed member through test(cycles=True).  The curated cases
(tests/ledger_cycle_histories.py) are the smallest at which a kernel can go wrong: a 3-cycle through three partial reads that no other
member decides; a cycle through clean reads only; the equal-class cases, each on its own, with clean reads exactly on a component's
lo and hi class, inside it and outside by the realtime tie; 63 / 64 / 65 reads; cores of 0, 1, 31, 32, 33, 63, 64 and 65 reads (the
matrix's word edges); a core path of 70 closed into one cycle (at least 7 squarings) and left open; two components; all-complete
histories, valid, forked and regressed, held to tbc_ledger_snapshots and tbc_ledger_realtime in the same test; reads without an
invocation, reads that check nothing, negative counters, equal sums with unequal partial vectors; 200 random histories; a core above
the cap.  References are computed once."""
import random

import numpy as np
import pytest

import ledger_cycle_histories as CH
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import ledger as L
from test_ledger_cycles_host import assert_same

pytestmark = pytest.mark.gpu

CASES = CH.cases()


def device(history, opts):
    cols = L.LedgerColumns(history)
    return cols, L.check_cycles_native(cols, opts["accounts"])


@pytest.fixture(scope="module")
def refs(native):
    return {c["name"]: L.cycles_numpy(c["history"], c["opts"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_numpy_statement(refs, case):
    h, o = case["history"], case["opts"]
    want = refs[case["name"]]
    for k, v in case["counts"].items():                                        # the case has the shape it was built for
        assert want["summary"][k] == v, (case["name"], k)
    cols, got = device(h, o)
    assert_same(got, want, case["name"])
    if want["summary"]["read_count"] <= 64:
        assert_same(got, L.cycles_host(h, o), case["name"], rounds=False)
    assert got["summary"]["n_checked"] == want["summary"]["n_checked"] > 0
    assert L.cycles_result_map(h, cols, got, o["accounts"]) == L._cyc_map(h, want, o["accounts"])


def test_the_three_partial_cycle_passes_the_snapshot_member_inexactly(refs):
    case = next(c for c in CASES if c["name"] == "three-partial-cycle")
    h, o = case["history"], case["opts"]
    cols = L.LedgerColumns(h)
    snap = L.snapshots_result_map(h, cols, L.check_snapshots_native(cols, o["accounts"]), o["accounts"])
    assert snap["valid?"] is True and snap["exact?"] is False
    t = L.test(dict(o), cycles=True, snapshots=True)
    res = t["checker"].check(t, h, {})
    assert res["snapshots"]["valid?"] is True and res["cycles"]["valid?"] is False and res["cycles"]["exact?"] is True
    assert res["cycles"]["on-cycle-count"] == 3 and len(res["cycles"]["witness"]) == 3


def test_the_closure_of_the_path_of_70_takes_seven_squarings_at_least(refs):
    got = device(*[next(c for c in CASES if c["name"] == "core-path-of-70-closed")[k] for k in ("history", "opts")])[1]
    assert got["summary"]["closure_rounds"] == refs["core-path-of-70-closed"]["summary"]["closure_rounds"] >= 7


@pytest.mark.parametrize("name", ["all-complete-valid", "all-complete-long-fork", "all-complete-regressed"])
def test_all_complete_histories_agree_with_snapshots_and_realtime(refs, name):
    case = next(c for c in CASES if c["name"] == name)
    h, o = case["history"], case["opts"]
    cols, got = device(h, o)
    assert got["summary"]["n_partial"] == 0
    snap = L.check_snapshots_native(cols, o["accounts"])
    accounts, init, apply_ok = L._rt_opts(None, o)
    rt = L.check_realtime_native(cols, accounts, init, apply_ok)
    bad = (snap["count"] > 0) | ((rt["bits"] & 48) != 0)
    assert bool(got["summary"]["n_on_cycle"]) == bool(bad.any()) == (name != "all-complete-valid")
    assert ((got["flags"][bad] & L.CYC_ON_CYCLE) != 0).all()
    for r in np.flatnonzero(snap["count"]):
        assert got["scc"][r] == got["scc"][snap["first"][r]] != N.NO_OP
    if name == "all-complete-valid":
        assert got["summary"]["n_core"] == 0 and got["summary"]["closure_rounds"] == 0 and got["summary"]["valid"] == 1


def test_random_histories(native):
    rng = random.Random(31)
    on_cycle = 0
    for trial in range(200):
        h, o = CH.random_history(rng)
        want = L.cycles_numpy(h, o)
        got = device(h, o)[1]
        assert_same(got, want, (trial, h, o))
        on_cycle += want["summary"]["n_on_cycle"] > 0
    assert 40 <= on_cycle <= 190


def test_more_reads_than_a_step_of_the_scans(native):
    """past 256 reads the one-workgroup scans carry from step to step; past 256 core reads a row of the matrix takes several steps"""
    rng = random.Random(4)
    accounts, rows = CH.core_path(300, True, 2)
    rows = rows[:150] + [CH.full(accounts, 9 + k // 2) for k in range(30)] + rows[150:]
    h, o = CH.concurrent(accounts, rows)
    want = L.cycles_numpy(h, o)
    assert want["summary"]["n_core"] == 300 and want["summary"]["n_on_cycle"] == 300
    assert_same(device(h, o)[1], want, "300")
    rows = [CH.full([1, 2], k // 3) for k in range(3000)]
    for k in rng.sample(range(3000), 90):
        rows[k] = [(1, rng.randrange(1000), rng.randrange(1000))]
    h, o = CH.timed_reads([1, 2], [(row, 2 * k, 2 * k + 1) for k, row in enumerate(rows)])
    want = L.cycles_numpy(h, o)
    assert want["summary"]["n_partial"] == 90 and want["summary"]["n_on_cycle"] > 90
    assert_same(device(h, o)[1], want, "3000")


def test_a_core_above_the_cap_is_unsupported_with_its_size(native):
    n = L.CYCLES_MAX_CORE + 1
    h, o = CH.timed_reads([1, 2], [([(1, 5, 5)], 2 * k, 2 * k + 1) for k in range(n)])       # partial reads only, one micro-op each: valid, no cycle
    cols = L.LedgerColumns(h)
    got = L.check_cycles_native(cols, o["accounts"])
    assert got.get("unsupported") and got["summary"]["n_core"] == n and got["summary"]["read_count"] == n and got["summary"]["n_partial"] == n
    assert L.cycles_result_map(h, cols, got, o["accounts"]) == {"valid?": "unknown", "searched?": False, "n-core": n}
    s, keep = L.ledger_rt_in(cols, o["accounts"], {a: (0, 0) for a in o["accounts"]})
    import ctypes as C
    out = N.LedgerCyclesOut()
    assert N.lib().tbc_ledger_cycles(C.byref(s), C.byref(out)) == N.ERR_UNSUPPORTED and out.summary.n_core == n
    assert "16384 at most" in N.lib().tbc_last_error().decode()


def test_bad_arguments_are_refused_before_any_device_call(native):
    import ctypes as C
    h, o = CASES[0]["history"], CASES[0]["opts"]
    cols = L.LedgerColumns(h)
    s, keep = L.ledger_rt_in(cols, o["accounts"], {a: (0, 0) for a in o["accounts"]})
    out = N.LedgerCyclesOut()
    assert N.lib().tbc_ledger_cycles(None, C.byref(out)) == N.ERR_INVALID_ARG
    s.process = None
    assert N.lib().tbc_ledger_cycles(C.byref(s), C.byref(out)) == N.ERR_INVALID_ARG
    assert "tbc_ledger_cycles: null argument (process)" in N.lib().tbc_last_error().decode()

"""CPU only: the oracles' own statements of TBC_MODEL_MUTEX and TBC_MODEL_TABLE (oracle_model.h, wgl_ref.c, wgl_window.c, wgl_beam.c,
sweep_ref.c, linear_ref.c) against the definition (oracle/brute.py) on small seeded histories, and against one another on the medium
shapes the device tests use (tests/model_histories.py) -- what tests/test_models_gpu.py compares the kernels with is pinned here first."""
import pytest

import model_histories as MH
from helpers import op_tuples
from oracle import brute

NARROW = dict(round_pairs=8, rules_at_any_round_size=True, branch_lists=True)


def _small(family, seed):
    bad = seed % 2 == 1
    if family in ("mutex", "mutex-held"):
        hist = MH.mutex_history(8, 3 + seed % 2, seed, busy=0.8, info=0.15, corrupt=MH.MUTEX_CORRUPT if bad else None,
                                held_at_start=family == "mutex-held")
        return (hist,) + MH.encode_mutex(hist, held=family == "mutex-held")
    if family == "table":
        start = 2 + seed % 3
        hist = MH.table_history(8, 3 + seed % 2, seed, busy=0.8, info=0.15, corrupt=bad, start=start)
        return (hist,) + MH.encode_table(hist, MH.table_model(start))
    hist = MH.set_table_history(8, 3 + seed % 2, seed, busy=0.8, info=0.15, corrupt=bad, n_elems=3)
    return (hist,) + MH.encode_set_table(hist)


@pytest.mark.parametrize("family", ["mutex", "mutex-held", "table", "set-table"])
def test_small_histories_against_brute_force(native, oracle, family):
    """Every CPU statement of the search gives the definition's verdict and its failing op; every witness is a legal run."""
    n_bad = n_ok = n_inv = n_kept = 0
    N_SEEDS = 200
    for seed in range(N_SEEDS):
        hist, enc, om = _small(family, 3000 + seed)
        d, tup = enc.ops.as_dict(), op_tuples(enc.ops)
        n_inv += sum(1 for o in hist if o["type"] == "invoke")
        n_kept += len(tup)
        bad = brute.first_bad_completion(om, tup)
        n_bad += bad is not None
        n_ok += bad is None
        want = (1, None) if bad is None else (0, bad)
        runs = {"window": oracle.check(d, om, "window"), "ref": oracle.check(d, om, "ref"),
                "beam1": oracle.check_beam(d, om, 1), "beam4": oracle.check_beam(d, om, 4), "narrow": oracle.check_beam(d, om, 1, **NARROW),
                "sweep": oracle.check_sweep(d, om, seg_target=0), "linear": oracle.check_linear(d, om)}
        for name, r in runs.items():
            assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == want, (family, seed, name, r["valid"], r["fail_op"], want)
            if bad is None and r.get("witness") is not None:
                assert brute.check_witness(om, tup, [int(x) for x in r["witness"]]) == r["final_state"], (family, seed, name)
    assert 5 * n_bad >= N_SEEDS and 5 * n_ok >= N_SEEDS, (family, n_bad, n_ok)
    assert 2 * n_kept >= n_inv, (family, n_kept, n_inv)          # failed calls disappear: at least half of the invocations are ops


def test_the_mutex_corruption_kept_is_the_one_found_invalid_more_often(native, oracle):
    """mutex_history has two ways to spoil a history; MUTEX_CORRUPT names the one that is used.  Counted here over the small
    histories: an open crashed :release explains either, and the second :acquire is explained less often than the lost :release."""
    found = {}
    for how in ("double-acquire", "lost-release"):
        found[how] = 0
        for seed in range(200):
            hist = MH.mutex_history(8, 3 + seed % 2, 5000 + seed, busy=0.8, info=0.15, corrupt=how)
            enc, om = MH.encode_mutex(hist)
            found[how] += oracle.check(enc.ops.as_dict(), om, "window", want_witness=False)["valid"] == 0
    assert max(found, key=found.get) == MH.MUTEX_CORRUPT, found


# Shapes the level sweep cannot reach: every crashed call that is open doubles a level's set of configs, and these valid histories keep
# 24 to 82 crashed :acquire / :release calls open to the end (levels past 300,000 configs; sweep_ref.c gives up there or runs for minutes).
# Every other shape, crashed or not, at any mask width, is swept: the device's own limits (one mask word, 64 calls open, 512 configs a
# level) belong to tests/test_models_gpu.py, not here.
SWEEP_OUT_OF_REACH = ("mutex-2-crashes", "mutex-4-crashes")
SWEEP_MAX_LEVEL = 300_000


def test_medium_shapes_the_oracles_agree(native, oracle):
    """Every shape of tests/model_histories.py x two seeds (each mask width, with and without crashed calls, valid and corrupted; the
    shape itself is asserted by references()): the sequential and the wide (2, 8, 16 configs a round) oracle give one verdict and one
    failing op on all of them, the sweep oracle on all but the two shapes named in SWEEP_OUT_OF_REACH; none runs into its limit."""
    cases = MH.references(oracle)
    assert len(cases) == len(MH.SHAPES) * len(MH.SEEDS)
    assert {MH.mask_words(c.ops) for c in cases if c.is_mutex} == {1, 2, 4, 8} == {MH.mask_words(c.ops) for c in cases if c.model == "table"}
    n_swept = 0
    for c in cases:
        want = (c.ref["valid"], c.ref["fail_op"] if c.ref["valid"] == 0 else None)
        for width in (2, 8, 16):
            r = oracle.check_beam(c.d(), c.om, width, max_probes=MH.MAX_PROBES, want_witness=False)
            assert r["valid"] != -1, (c.name, width)
            assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == want, (c.name, width)
        if c.name.split("/")[0] in SWEEP_OUT_OF_REACH:
            assert c.crashed >= 20 and c.ref["valid"] == 1, (c.name, c.crashed)          # (the stated reason holds)
            continue
        s = oracle.check_sweep(c.d(), c.om, seg_target=0, max_level=SWEEP_MAX_LEVEL)
        assert s["valid"] != -1, (c.name, s["max_level"])
        assert (s["valid"], s["fail_op"] if s["valid"] == 0 else None) == want, (c.name, "sweep")
        n_swept += 1
    assert n_swept == len(cases) - len(SWEEP_OUT_OF_REACH) * len(MH.SEEDS)

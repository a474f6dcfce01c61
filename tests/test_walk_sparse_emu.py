"""The sparse form of the front walk's phase C (csrc/open_walk_impl.h) -- the set of calls open at a front as the prefix-XOR over the fronts
of ON / OFF toggle events, list entries and twin masks per front, the producer distance from byte counters of invocation ranks; no loop
over the candidates with lane = front -- on the CPU under the lane-accurate emulator of tests/emu, in the run form the kernel launches,
against the host-built tables word for word (tests/emu/host_tables.h).  Beside the words: every chunk of the <8> instantiation takes the
form (wv::stat), three planted mutations of it are seen, and the dense loop it replaces still gives the same words.  Test infrastructure
only: the product has no CPU path."""
import functools

import pytest

from emu import walk_runs, walk_sparse
from jepsen_tigerbeetle_amd import synth

import walk_sparse_shapes as shapes

K = walk_runs.run_length()


@functools.lru_cache(maxsize=None)
def _small():
    return shapes.small_shapes(K)


@functools.lru_cache(maxsize=None)
def _hand():
    return shapes.hand_built()


def _check(hists, vpad=8, run=K, sparse=True, **kw):
    bad, n = walk_sparse.check(hists, vpad, run=0 if run == K else run, dense=not sparse, **kw)
    assert bad is None, bad
    assert n["mismatches"] == 0, n
    runs, chunks = walk_runs.expected_counts(hists, run)
    assert n["searches"] == runs and n["carried"] == chunks - runs, (n, runs, chunks)
    assert n["nc_le64"] + n["nc_mid"] + n["nc_more"] == chunks, n
    # (a chunk of more candidates than the form's round buffer leaves room for in the table keeps the dense loop)
    assert (n["sparse"], n["dense"]) == ((chunks - n["nc_more"], n["nc_more"]) if sparse and vpad <= 8 else (0, chunks)), n
    return n


@pytest.mark.parametrize("order", [0, 1, 2, 16, 16 + 24])
def test_every_word_in_every_order(order):
    """the headline's format (compact records, branch lists, twin masks, lookahead) in orders slot / completion / writes last / 16 / 40"""
    n = _check(_small(), branch=True, front="compact", by_ret=order)
    assert n["nc_le64"] and n["nc_mid"] and n["nc_more"], n           # one and two passes of 64 candidates; too many for the form


@pytest.mark.parametrize("front,branch,twin,look", [("plain", False, True, True), ("wide", False, True, True), ("wide", True, True, True),
                                                    ("compact", True, False, True), ("plain", False, True, False), ("plain", False, False, False)])
def test_formats_and_optional_tables(front, branch, twin, look):
    """plain rows and wide records, full lists (reads are list entries, more than 8 a front), no twin masks, no lookahead"""
    for order in (0, 16 + 24):
        _check(_small(), front=front, branch=branch, twin=twin, look=look, by_ret=order)


@functools.lru_cache(maxsize=None)
def _count_form():
    return shapes.count_form_shapes()


@pytest.mark.parametrize("order", [0, 1, 2, 16, 16 + 24])
def test_count_form_with_slotless_crashed_calls(order):
    """the count form: live calls on re-used slots, crashed calls on none -- a slot handed from one process to the next on one front, with
    the crashed call between them in no record list.  lst, twn, rdm and look, every word (look word 0 without the bit that is not the walk's)"""
    hs = _count_form()
    for kw in (dict(branch=True, front="compact"), dict(branch=False, front="plain")):
        bad, n = walk_sparse.check(hs, 8, by_ret=order, count_form=True, **kw)
        assert bad is None, (kw, bad)
        assert n["mismatches"] == 0 and n["dense"] == 0 and n["sparse"] == n["chunks"] == n["searches"] + n["carried"], n


def test_count_form_sees_the_planted_mutations():
    for mutation in ("off_at_ret", "twin_le"):
        bad, _ = walk_sparse.check(_count_form(), 8, branch=True, front="compact", by_ret=16 + 24, count_form=True, mutation=mutation)
        assert bad is not None, mutation


def test_sixty_four_slots_on_the_sparse_form():
    """calls on slots 0 .. 63 with few enough candidates a chunk: the high toggle words and the second scan, by hand"""
    n = _check([shapes.sixty_four_sparse()], branch=True, front="compact", by_ret=16 + 24)
    assert n["dense"] == 0 and n["sparse"] >= 5, n


def test_no_rows_at_all():
    _check(_hand(), vpad=0, twin=False, look=False, front="plain")


@pytest.mark.parametrize("run", sorted({2, 3} - {K}))
def test_other_run_lengths(run):
    _check(shapes.hand_built() + shapes.runs_shapes.chunk_counts(run), run=run, branch=True, front="compact", by_ret=16 + 24)


def test_the_dense_loop_still_agrees():
    """what rows of more than 8 entries and a chunk that overflows the candidate table take: the same words at 8 entries, and rows of 32"""
    _check(_hand(), sparse=False, branch=True, front="compact", by_ret=16 + 24)
    _check(_hand(), sparse=False, front="plain")
    hs = [shapes.runs_shapes.gen(300, 24, 0.6, seed=1, n_values=31), shapes.handover(3, 100)]
    _check(hs, vpad=32, front="plain")


@pytest.mark.parametrize("mutation,what", [("off_at_ret", {"lst", "rdm", "look mask"}), ("twin_le", {"twn"}), ("no_self_exclusion", {"look word 0"})])
def test_planted_mutations_are_seen(mutation, what):
    """OFF at ret instead of ret + 1; ret_u <= ret_c in the twin test; the completing call counted as a producer of what it needs"""
    seen = set()
    for order in (0, 16 + 24):
        bad, _ = walk_sparse.check(_hand(), 8, branch=True, front="compact", by_ret=order, mutation=mutation)
        assert bad is not None, (mutation, order)
        seen.add(bad[0])
    assert seen <= what, seen


def test_cas_v_v_alone_is_what_the_self_exclusion_is_for():
    """without another producer the only invocation in the window is the call's own: the mutation shows there, and at no other hand-built shape
    would the test of it be as narrow"""
    bad, _ = walk_sparse.check([shapes.cas_v_v(False)], 8, branch=True, front="compact", mutation="no_self_exclusion")
    assert bad is not None and bad[0] == "look word 0", bad
    bad, _ = walk_sparse.check([shapes.cas_v_v(True)], 8, branch=True, front="compact", mutation="no_self_exclusion")
    assert bad is None, bad        # (two invocations at that rank: the distance is the same with or without the call's own)


def test_bench_shaped_histories_take_the_sparse_form_in_every_chunk():
    """two of the bench's histories (10k invocations, 64 processes) in the headline's format and order"""
    hs = synth.register_ops_many(range(7000, 7002), n_ops=10000, n_procs=64, busy=0.1, info=0.0)
    n = _check(hs, branch=True, front="compact", by_ret=16 + 24)
    assert n["dense"] == 0 and n["sparse"] > 200 and n["emit_trips"] < 20 * n["sparse"] and n["rounds"] < 16 * n["sparse"], n

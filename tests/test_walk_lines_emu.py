"""The sparse form's list stores with LANE = ENTRY (csrc/open_walk_impl.h, sparse_lists: the fronts leave their sets of open listed calls in
the round buffer, a chunk's entries are taken 64 at a time, an entry lane finds its front, its rank k within it and the k-th set bit of the
front's words) on the CPU under the lane-accurate emulator of tests/emu: the run form the kernel launches and every chunk once more from
nothing, against the host-built tables word for word (tests/emu/host_tables.h).  Beside the words, per chunk: the passes of 64 entries it
makes are ceil(entries / 64), its entries are off[F_hi] - off[F_lo], and every front's off[] is the running sum of the counts before it
(a chunk's entries are one contiguous piece of lst / twn).  Two planted mutations of the form are seen.  Test infrastructure only: the
product has no CPU path."""
import functools

import pytest

from emu import walk_lines

import walk_lines_shapes as shapes


@functools.lru_cache(maxsize=None)
def _hand():
    return shapes.hand_built()


def _check(hists, **kw):
    bad, n, entries, sparse = walk_lines.check(hists, **kw)
    assert bad is None, bad
    assert n["mismatches"] == 0, n
    # one pass of 64 entries per 64 entries begun, chunk by chunk; the chunk's entries are the tables'; contiguous; every entry has its candidate
    assert n["chunks_off"] == 0 and n["passes"] == n["passes_expected"] and n["entries"] == n["entries_expected"], n
    assert n["fronts_apart"] == 0 and n["no_candidate"] == 0, n
    assert n["passes_expected"] == sum((e + 63) // 64 for e, s in zip(entries, sparse) if s), n
    return n, entries, sparse


@pytest.mark.parametrize("order", [0, 1, 2, 16, 16 + 24])
def test_every_word_and_every_pass_in_every_order(order):
    """the headline's format (compact records, branch lists, twin masks, lookahead) in orders slot / completion / writes last / 16 / 40"""
    n, entries, sparse = _check(_hand(), branch=True, front="compact", by_ret=order)
    assert n["second_set"] > 0, n                                   # a front with entries from the second set of 64 places
    # the first history's chunks have no entry at all, 1, 63, 64 and 65, and none in the last chunk of ten fronts; the second's 127 and 128
    assert entries[:6] == [0, 1, 63, 64, 65, 0] and all(sparse[:6]), entries[:8]
    assert entries[6:9] == [127, 128, 128], entries[6:10]
    # a dense chunk between two sparse ones of one run
    i = sparse.index(0)
    assert sparse[i - 1:i + 2] == [1, 0, 1] and entries[i] > 101, (i, sparse, entries)


def test_the_shapes_count_what_they_say():
    """the definition's entries per chunk (Python) are the host tables' (off[])"""
    _, _, entries, _ = walk_lines.check(_hand(), branch=True, front="compact")
    want = [e for h in _hand() for e in shapes.entries_per_chunk(h)]
    assert entries == want


@pytest.mark.parametrize("front,branch,twin,look", [("wide", True, True, True), ("wide", False, True, True), ("compact", True, False, True),
                                                    ("plain", False, False, False)])
def test_formats_and_twin_masks_off(front, branch, twin, look):
    """wide records and plain rows, full lists (a read is an entry: no empty front), no twin masks, no lookahead"""
    for order in (0, 16 + 24):
        _check(_hand(), front=front, branch=branch, twin=twin, look=look, by_ret=order)


def test_count_form_with_reused_slots():
    """live calls on re-used slots, crashed calls on none: a slot handed from one process to the next inside a chunk"""
    hs = [shapes.sparse_shapes.slots_handed_on()]
    for order in (0, 16 + 24):
        bad, n, _, sparse = walk_lines.check(hs, branch=True, front="compact", by_ret=order, count_form=True)
        assert bad is None, bad
        assert all(sparse) and n["chunks_off"] == 0 and n["passes"] == n["passes_expected"] > 0 and n["fronts_apart"] == 0 and n["no_candidate"] == 0, n


@pytest.mark.parametrize("mutation", ["rank_off_by_one", "front_le"])
def test_planted_mutations_are_seen(mutation):
    """the rank within the front one too high; `<=` for `<` where a front's first entry is looked for in a pass, so that a front beginning with the
    pass is not found there.  Each changes list words, and entries are left without a candidate"""
    for order in (0, 16 + 24):
        bad, _, _, _ = walk_lines.check(_hand(), branch=True, front="compact", by_ret=order, mutation=mutation)
        assert bad is not None and bad[0] in ("lst", "twn"), (mutation, order, bad)
    # the boundary alone: two entries at every front, so that front 32 of the second chunk begins with its second pass
    bad, _, _, _ = walk_lines.check([shapes.two_at_every_front()], branch=True, front="compact", mutation="front_le")
    assert bad is not None and bad[0] == "lst" and bad[2] >= 64, bad

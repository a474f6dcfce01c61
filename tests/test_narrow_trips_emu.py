"""K5n's dependent memory trips, counted on the CPU.  A round of the narrow kernel is meant to be two dependent trips: the child's
front record with the lookahead records, then the child's bucket with the next candidates.  Three paths written as exceptions added
about one more per wave iteration on the bench workload -- the lookahead for children 16 and up, claim passes lost to a neighbour's
bucket sharing a claim word, a byte pair per rank past a front record's window.  The kernel body counts them (wv::stat ids 29 and up
in csrc/wgl_narrow_impl.h, nothing on the device); here the emulator runs the very body and the counts are pinned, next to the
oracle's answer for every history (tests/test_narrow_emu.py's compare).

Counts under the body as it was before (same inputs; profiles/NOTES_narrow_trips.md has the whole table), bench shape: of 6,537
wave iterations 2,982 loaded a lookahead batch after the first wait, 2,336 claim passes were second or later ones (2,142 lanes
lost a claim, 5 of them to a lane that wanted the same entry), 1,538 lanes loaded a byte pair past the window."""
import ctypes as C

import pytest

import emu
from jepsen_tigerbeetle_amd import columns, synth
from test_narrow_emu import CAS, compare

# csrc/wgl_narrow_impl.h, S_*
ITER, NN16, NN24, NN32, LOOK_LATE, CLAIM_PASS, CLAIM_AGAIN, LOSE_TRUE, LOSE_FALSE, NEXT_BUCKET, WINDOW = range(29, 40)


def stats(reset=True):
    out = (C.c_uint64 * 64)()
    emu.lib().emu_stats(out, C.c_int(1 if reset else 0))
    return list(out)


def counted(hists, L=8, **kw):
    """compare() with the oracle, and the stat counters of that run alone"""
    stats()
    got = compare(hists, CAS, L, **kw)
    return got, stats()


def check_trips(s):
    """what holds on every input: the rare paths that are left are the ones that must be"""
    assert s[LOOK_LATE] <= 4 * s[NN32] and (s[NN32] > 0 or s[LOOK_LATE] == 0)      # a lookahead load after the first wait only past 32 children
    assert s[LOSE_FALSE] == 0                                                        # nobody loses an entry to a lane busy with another bucket
    assert s[CLAIM_AGAIN] <= s[LOSE_TRUE] + s[NEXT_BUCKET]
    assert s[CLAIM_PASS] == s[ITER] + s[CLAIM_AGAIN]


@pytest.fixture(scope="module")
def small():
    """16 histories at ~8 calls in flight: one wavefront's two sets of eight"""
    return [columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.5, seed=s)) for s in range(100, 116)]


def test_bench_shape_common_round_makes_no_rare_trip():
    """8 bench-shaped histories, one wavefront, the bench's options (compact records, 4 entries per op, no witness, the shipped list order)"""
    hists = synth.register_ops_many(range(7000, 7008), n_ops=10000, n_procs=64, busy=0.1)
    got, s = counted(hists, tag="trips-bench", entries_per_op=4, pool_words=8_000_000, want_witness=False, by_ret=16 + 24, max_waves=1)
    assert all(g["valid"] == 1 for g in got)
    check_trips(s)
    assert s[ITER] == 6537 and sum(g["probes"] for g in got) == 85882 and sum(g["bucket_reads"] for g in got) == 37772      # the schedule is the oracle's: so are these
    assert (s[NN16], s[NN24], s[NN32]) == (2982, 56, 0) and s[LOOK_LATE] == 0
    assert (s[LOSE_TRUE], s[NEXT_BUCKET]) == (5, 935)
    assert s[CLAIM_AGAIN] <= 940
    # one load per seven ranks past the window, where the bytes were a load pair per rank (1,538 of them)
    assert s[WINDOW] == 778


def test_every_path_is_taken_at_a_small_shape(small):
    """the paths are exercised, not correct by being absent: more than 16 and 24 children, a window reload, true claim conflicts,
    full buckets -- with the bench's options, then with first sets of one entry per op and lists in slot order"""
    got, s = counted(small, tag="trips-small", entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1)
    check_trips(s)
    assert s[NN16] > 0 and s[NN24] > 0 and s[WINDOW] > 0 and s[LOSE_TRUE] > 0 and s[NEXT_BUCKET] > 0, s[ITER:WINDOW + 1]
    assert (s[NN16], s[NN24], s[WINDOW], s[LOSE_TRUE], s[NEXT_BUCKET]) == (174, 7, 75, 14, 73)
    got, s = counted(small, tag="trips-small-slot", entries_per_op=1, pool_words=8_000_000, max_waves=1)
    check_trips(s)
    assert s[NN16] > 0 and s[WINDOW] > 0 and s[LOSE_TRUE] > 0 and s[NEXT_BUCKET] > 0, s[ITER:WINDOW + 1]
    assert s[NEXT_BUCKET] == 81
    # (no set grows at this shape: a first set has 1,024 entries at least and these histories insert ~350 configs each --
    # growth beside the claims is test_sets_that_grow_keep_the_claims_exact)
    assert all(g["tab_log2"] == 10 for g in got)
    # ... without a witness (no parent links) and as two wavefronts
    got, s = counted(small, tag="trips-small-nolinks", entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, want_witness=False)
    check_trips(s)


def test_more_than_32_children_keep_the_loop(small):
    """nn0 > 32.  With both dominance rules on no shape tried reaches it under the emulator (16 processes at duty 0.8, 16 histories:
    0 of 2,961 iterations; 32 processes: 0 of 2,081; the bench shape: 0 of 6,537) -- the rules leave a group two or three viable
    children a round.  With the rules off the same 16 histories do (5 iterations), and with the eager rule alone at duty 0.8 the loop
    runs twice in one iteration (more than 40 children): the loop past 32 is covered there, a step limit keeping it to seconds."""
    got, s = counted(small, tag="trips-rules-off", rules=0, entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1, want_witness=False)
    check_trips(s)
    assert s[NN32] > 0 and s[LOOK_LATE] >= s[NN32]
    busy = [columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.8, seed=sd)) for sd in range(100, 116)]
    got, s = counted(busy, tag="trips-busy", entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1, want_witness=False, max_steps=20000)
    check_trips(s)
    assert s[NN32] == 0 and s[NN24] > 0
    got, s = counted(busy, tag="trips-busy-eager-only", rules=1, entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1, max_steps=20000)
    check_trips(s)
    assert s[NN32] > 0 and s[LOOK_LATE] > s[NN32]


def test_sets_that_grow_keep_the_claims_exact():
    """first sets of one entry per op that the histories outgrow inside the kernel (the claim words are only valid within a pass: a
    grown set has new entry numbers), in slot order"""
    hists = [columns.pair_events(synth.register_events(n_ops=2500, n_procs=16, seed=sd, busy=0.25)) for sd in range(4)]
    got, s = counted(hists, tag="trips-grow", entries_per_op=1, pool_words=8_000_000, max_waves=1, want_witness=False)
    check_trips(s)
    assert sum(g["tab_log2"] > 12 for g in got) >= 2 and s[NEXT_BUCKET] > 0


def test_wider_masks_keep_two_batches_in_trip_1():
    """two mask words (more than 64 process slots): their kernels have no registers for two more batches (csrc/wgl_narrow_impl.h, NB), so
    children past 16 are loaded in the loop as before -- counted as such; claims and answers as with one word"""
    hists = [columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.5, seed=sd)) for sd in range(100, 116)]
    stats()
    got = compare(hists, CAS, 8, tag="trips-mw2", mw=2, entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1)
    s = stats()
    assert s[NN16] == 174 and s[LOOK_LATE] == 174 + 7 and s[LOSE_FALSE] == 0 and s[LOSE_TRUE] > 0      # (another hash than with one word: other conflicts)
    assert s[CLAIM_AGAIN] <= s[LOSE_TRUE] + s[NEXT_BUCKET]


@pytest.mark.parametrize("L", [4, 16, 32])
def test_other_group_sizes_claim_and_look_the_same_way(small, L):
    """a claim word per lane of the group, whatever the group's size; 16 groups of 4 lanes reach 32 children with the rules on"""
    got, s = counted(small, L=L, tag="trips-L", entries_per_op=4, pool_words=8_000_000, by_ret=16 + 24, max_waves=1, want_witness=False)
    check_trips(s)
    wide = [columns.pair_events(synth.register_events(n_ops=300, n_procs=16, busy=0.5, seed=sd, n_values=9)) for sd in range(100, 108)]      # values 0..8: the 128 B records
    got, s = counted(wide, L=L, tag="trips-L-wide-records", entries_per_op=4, pool_words=8_000_000, max_waves=1)
    check_trips(s)
    assert s[WINDOW] == 0                                                            # (those records carry 16 ranks; past them bytes, as ever)

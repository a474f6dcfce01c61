"""Histories for the tests of the sparse form's list stores with lane = entry (tests/test_walk_lines_emu.py on the CPU,
tests/test_walk_lines_gpu.py on the device): the smallest shapes at which taking a chunk's list entries 64 at a time -- an entry lane finds its
front and its rank within it, then the rank-th open call of the front -- can go wrong.  The counts named below hold under BRANCH LISTS (a read
is no list entry), which is the headline's format."""
import numpy as np

from jepsen_tigerbeetle_amd import _native as N

import walk_sparse_shapes as sparse_shapes

W, R, CAS = N.F_WRITE, N.F_READ, N.F_CAS
hand = sparse_shapes.hand


def entries_per_chunk(h, branch=True):
    """list entries of each chunk of 64 fronts, from the definition: front F is the F-th completion, and a completed call (under branch lists:
    not a read) is an entry of every front from the completions before its invocation to its own"""
    f, inv, ret = np.asarray(h.f), np.asarray(h.inv_pos, np.int64), np.asarray(h.ret_pos, np.int64)
    done = ret != 0xFFFFFFFF
    rets = np.sort(ret[done])
    n = np.zeros(len(rets) + 1, np.int64)
    for i in np.nonzero(done & ((f != R) | (not branch)))[0]:
        n[np.searchsorted(rets, inv[i])] += 1
        n[np.searchsorted(rets, ret[i]) + 1] -= 1
    per_front = np.cumsum(n)[:len(rets)]
    return [int(per_front[c:c + 64].sum()) for c in range(0, len(rets), 64)]


def counted_chunks():
    """one process, a call at a time -- a :write is the one entry of its front, a read's front has none -- so that the chunks have exactly
    0, 1, 63, 64 and 65 entries, then a last chunk of 10 fronts without any: all reads; one write among reads (empty fronts on both sides of
    a full one); 63 writes round a read (an empty front between full ones); 64 writes; 63 writes and a second process's write that is
    open at one of their fronts and completes on a front of its own (64 fronts, 65 entries: the 65th is alone in a second pass)"""
    kinds = [R] * 64 + [R] * 30 + [W] + [R] * 33 + [W] * 40 + [R] + [W] * 23 + [W] * 64 + [W] * 63 + [R] * 10
    calls = [(0, j + 0.1, j + 0.6, k, 1 + j % 4, 0) for j, k in enumerate(kinds)]
    calls.append((1, 300.5, 300.7, W, 2, 0))
    h = hand(calls)
    assert entries_per_chunk(h) == [0, 1, 63, 64, 65, 0], entries_per_chunk(h)
    return h


def two_at_every_front(n=100, cas_every=0):
    """two processes whose calls overlap so that each is open when the other's completes: two entries at every front but the first.  The
    first chunk has 127 entries, the others 128: where the first has a front whose two entries are the last of a pass and the first of the
    next (entries 63 and 64), the second has a front that begins with a pass (entry 64).  cas_every: every so many-th call a :cas of the
    effect of its neighbours' (twin masks)"""
    calls = []
    for j in range(n):
        k = (CAS, 1, 2) if cas_every and j % cas_every == 0 else (W, 1 + j % 2, 0)
        calls.append((0, j - 0.3, j + 0.6) + k)
        calls.append((1, j + (0.2 if j else 0.65), j + 1.1) + k)       # (the very first front: the first process's call alone)
    h = hand(calls)
    e = entries_per_chunk(h)
    assert e[0] == 127 and e[1] == 128 and len(e) == (2 * n + 63) // 64, e
    return h


def dense_between_sparse():
    """three quick processes complete three calls a time unit; forty more invoke one long call each during the second chunk and complete it in
    the third: the second chunk has more than 101 candidates (its 71 completions and a call open on each of the forty slots) and keeps the
    dense loop, the first and the third -- chunks of the same run -- take the sparse form, and the third begins where the dense one left off"""
    calls = []
    for s in (0, 1, 2):
        for j in range(72):
            calls.append((s, j + 0.25 * s + 0.05, j + 0.25 * s + 0.65, (W, R, CAS)[(j + s) % 3], 1 + j % 4, 1 + (j + 1) % 4))
    for p in range(40):
        calls.append((3 + p, 22.0137 + 0.5 * p, 45.0071 + 0.37 * p, CAS if p % 3 == 0 else W, 1 + p % 3, 2))
    return hand(calls)


def hand_built():
    """what the form adds: the exact entry counts, two entries a front across pass boundaries, a dense chunk between sparse ones, twelve calls
    open at once with 65 - 101 candidates a chunk (places in the second set of 64), last chunks of 1 and 63 fronts"""
    return [counted_chunks(), two_at_every_front(), two_at_every_front(70, cas_every=3), dense_between_sparse(), sparse_shapes.crowded_front(),
            sparse_shapes.last_chunk_of(1), sparse_shapes.last_chunk_of(63)]


def generated(n=36):
    """histories of at most 512 ops: 3 - 64 processes, some with crashed calls"""
    hs = []
    for s in range(n):
        procs, busy = (3, 1.0) if s % 6 == 0 else (8, 0.6) if s % 6 == 1 else (16, 0.4) if s % 6 == 2 else (24, 0.5) if s % 6 == 3 else (64, 0.1) if s % 6 == 4 else (12, 0.9)
        hs.append(sparse_shapes.runs_shapes.gen(200 + 13 * (s % 24), procs, busy, info=0.02 if s % 4 == 3 else 0.0, seed=500 + s))
    assert all(len(h) <= 512 and h.n_process <= 64 for h in hs)
    return hs

"""Histories for the tests of the sparse form of the front walk's phase C (tests/test_walk_sparse_emu.py on the CPU,
tests/test_walk_sparse_gpu.py on the device): the smallest shapes at which membership by prefix-XOR of toggle events, the chain of a
call's twins, and the producer distance from byte counters of invocation ranks can go wrong."""
import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns

import walk_runs_shapes as runs_shapes

W, R, CAS = N.F_WRITE, N.F_READ, N.F_CAS


def hand(calls):
    """calls: (process, invoked at, completed at or None for a crashed call, f, a, b), times of any unit, all different.  Ops in order of
    invocation, positions = the order of the events."""
    events = sorted([(c[1], i, 0) for i, c in enumerate(calls)] + [(c[2], i, 1) for i, c in enumerate(calls) if c[2] is not None])
    assert len({t for t, _, _ in events}) == len(events)
    inv, ret = {}, {}
    for pos, (_, i, what) in enumerate(events):
        (ret if what else inv)[i] = pos
    order = sorted(range(len(calls)), key=lambda i: inv[i])
    procs = sorted({c[0] for c in calls})
    assert procs == list(range(len(procs)))
    return columns.OpColumns(f=np.array([calls[i][3] for i in order], np.uint8), a=np.array([calls[i][4] for i in order], np.int32),
                             b=np.array([calls[i][5] for i in order], np.int32), process=np.array([calls[i][0] for i in order], np.int32),
                             inv_pos=np.array([inv[i] for i in order], np.uint32), ret_pos=np.array([ret.get(i, 0xFFFFFFFF) for i in order], np.uint32),
                             n_events=len(events), n_process=len(procs))


def _fab(j):
    """write 1 .. 4, read (now and then of nil), cas: cycling"""
    kind = j % 3
    return ((W, R, CAS)[kind], 1 + j % 4 if kind != 1 else (N.NIL if j % 15 == 1 else 1 + (j // 3) % 4), 1 + (j + 1) % 4 if kind == 2 else 0)


def handover(n_procs, n_calls):
    """Every slot's next call is invoked straight after its last one completes -- no completion between: the call completes at rank r,
    the next is invoked at rank r + 1, i.e. the slot's OFF and ON events fall on the same front.  With n_procs slots and n_calls calls each
    that happens at every front of every chunk, the first and the last included."""
    step = 1.0 / (n_procs + 1)
    calls = []
    for p in range(n_procs):
        for k in range(n_calls):
            calls.append((p, k + step * p, k + step * p + 1.0 - step / 4) + _fab(len(calls)))
    return hand(calls)


def long_open():
    """slot 0: a write open from the 10th completion to the ~300th (ON at index 0 and no OFF in three whole chunks) while slots 1 - 3 complete
    three calls a time unit; then a few short calls on slot 0"""
    calls = [(0, 3.33, 100.07, W, 2, 0)] + [(0, 101.05 + j, 101.65 + j) + _fab(j) for j in range(6)]
    for s in (1, 2, 3):
        for j in range(108):
            calls.append((s, j + 0.25 * s, j + 0.25 * s + 0.6) + _fab(len(calls)))
    h = hand(calls)
    assert 320 < int((h.ret_pos != 0xFFFFFFFF).sum()) <= 384
    return h


def crashed_producer():
    """a crashed :write 3 (it keeps its slot and never completes) is the only producer of what later reads and cas calls need; a second
    crashed call, a :cas 1 -> 4, produces 4"""
    calls = [(0, 0.5, None, W, 3, 0), (1, 0.7, None, CAS, 1, 4)]
    for j in range(70):
        calls.append((2, 1.0 + j, 1.4 + j, R, 3, 0))
        calls.append((3, 1.2 + j, 1.7 + j, CAS, 3 if j % 2 else 4, 1))
        calls.append((4, 1.3 + j, 1.9 + j, W, 1, 0))
    return hand(calls)


def crowded_front():
    """twelve slots open at once (more than 8 list entries at every front of the middle), of which three :write 2, three :cas 1 -> 3 and two
    :write 5 share an effect, completing in an order that is not the slots'"""
    eff = [(W, 2, 0), (CAS, 1, 3), (W, 5, 0), (R, 2, 0), (W, 2, 0), (CAS, 1, 3), (R, N.NIL, 0), (W, 2, 0), (CAS, 1, 3), (W, 5, 0), (R, 1, 0), (CAS, 2, 2)]
    calls = []
    for k in range(8):                 # eight waves of twelve overlapping calls; later slots complete EARLIER within a wave
        for p, e in enumerate(eff):
            calls.append((p, 10.0 * k + 0.1 * p, 10.0 * k + 5.0 + 0.37 * ((7 * p + k) % 12) + 0.01 * p) + e)
    return hand(calls)


def cas_v_v(other_producer):
    """a :cas 3 -> 3 (it produces what it needs) completing at rank r + 1, invoked at rank r; with other_producer a :write 3 is invoked at the
    same rank r: the nearest OTHER producer is one rank back (and two calls were invoked at that rank); without it there is none, and the
    call's own invocation must not count.  Fillers before put the case at front 70 (the second chunk) and at front 3."""
    calls = []
    for base, n_fill in ((0.0, 3), (100.0, 66)):
        for j in range(n_fill):
            calls.append((0, base + j, base + j + 0.5, R, N.NIL, 0))
        t = base + n_fill
        calls.append((1, t + 0.10, t + 0.80, CAS, 3, 3))            # invoked at rank r
        if other_producer:
            calls.append((2, t + 0.20, t + 0.95, W, 3, 0))          # the same rank
        calls.append((0, t + 0.30, t + 0.50, R, N.NIL, 0))          # rank r completes; the cas completes at r + 1
        calls.append((0, t + 0.96, t + 0.99, W, 1, 0))
    return hand(calls)


def last_chunk_of(n):
    """a history whose last chunk has n fronts"""
    return runs_shapes._with_fronts(64 + n, seed=40 + n)


def sixty_four_slots():
    """exactly 64 process slots, all busy: slots 0 / 31 / 32 / 63, more than 128 candidates in a chunk"""
    h = handover(64, 5)
    assert h.n_process == 64
    return h


def sixty_four_sparse():
    """64 process slots of which ~6 are busy at a time: every chunk has few enough candidates for the sparse form, and calls sit on slots
    0 .. 63 -- the high words of the toggle buffer, the second scan of the slot rounds"""
    h = runs_shapes.gen(500, 64, 0.1, seed=22)
    assert h.n_process == 64 and int(np.asarray(h.process).max()) >= 48
    return h


def slots_handed_on():
    """For the COUNT FORM (crashed calls hold no slot, a process that crashes hands its slot back, the next new process takes the lowest
    free one): four lanes of twelve processes each.  A process completes four calls, then invokes a :write / :cas that never completes, and
    the next process of the lane invokes straight after that -- no completion between the last live call of one process and the first of
    the next, so a slot's OFF and ON events fall on one front with a slotless crashed call between them, at every part of three chunks.
    A fifth lane never crashes and keeps reading what only the crashed calls produce."""
    calls, proc = [], 0
    for lane in range(4):
        t = 0.013 * lane
        for k in range(12):
            for j in range(4):
                calls.append((proc, t + 0.05, t + 0.95) + _fab(len(calls)))
                t += 1.0
            calls.append((proc, t + 0.01, None, W if k % 2 else CAS, 1 + k % 4, 1 + (k + 1) % 4))
            t += 0.02
            proc += 1
    for j in range(45):
        calls.append((proc, 0.5 + j, 0.9 + j, R if j % 3 else CAS, 1 + j % 4, 2))
    h = hand(calls)
    assert h.n_process == 49 and int((h.ret_pos == 0xFFFFFFFF).sum()) == 48
    return h


def count_form_shapes():
    """the hand-built handing-on of slots, two generated histories with crashed calls (3 and 8 workers), and one without any"""
    hs = [slots_handed_on(), runs_shapes.gen(300, 3, 1.0, info=0.03, seed=31), runs_shapes.gen(400, 8, 0.6, info=0.04, seed=32), handover(3, 60)]
    assert all(h.n_process <= 64 for h in hs) and all((np.asarray(h.ret_pos) == 0xFFFFFFFF).sum() >= 5 for h in hs[:3])
    return hs


def hand_built():
    return [handover(3, 100), long_open(), crashed_producer(), crowded_front(), cas_v_v(True), cas_v_v(False), last_chunk_of(1), last_chunk_of(63),
            sixty_four_slots(), sixty_four_sparse()]


def small_shapes(run):
    """the hand-built cases above, then what the run form's tests use: a 1-op history, 64 and 65 ops, crashed calls that keep a slot, 2 - 3
    processes, 56 - 64 busy slots, a call open over four chunks, histories of 1, run - 1, run, run + 1 and 2 run + 1 chunks"""
    return hand_built() + runs_shapes.small_shapes(run)

"""Histories for the tests of the front walk's run form (tests/test_walk_runs_emu.py on the CPU, tests/test_walk_runs_gpu.py on the
device): the smallest shapes at which carrying a slot's cursor from one 64-front chunk to the next can go wrong."""
import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns, synth


def gen(n, p, busy, info=0.0, seed=1, **kw):
    return columns.pair_events(synth.register_events(n_ops=n, n_procs=p, seed=seed, busy=busy, info=info, **kw))


def by_hand(calls):
    """calls: (process, invoked at, completed at or None for a crashed call), times of any unit, all different.  Ops in order of
    invocation, positions = the order of the events; the functions and values cycle (write 1 .. 4, read, cas)."""
    events = sorted([(t0, i, 0) for i, (_, t0, _) in enumerate(calls)] + [(t1, i, 1) for i, (_, _, t1) in enumerate(calls) if t1 is not None])
    assert len({t for t, _, _ in events}) == len(events)
    inv, ret = {}, {}
    for pos, (_, i, what) in enumerate(events):
        (ret if what else inv)[i] = pos
    order = sorted(range(len(calls)), key=lambda i: inv[i])
    f, a, b = [], [], []
    for j, _ in enumerate(order):
        kind = j % 3
        f.append((N.F_WRITE, N.F_READ, N.F_CAS)[kind])
        a.append(1 + j % 4 if kind != 1 else (N.NIL if j % 15 == 1 else 1 + (j // 3) % 4))
        b.append(1 + (j + 1) % 4 if kind == 2 else 0)
    procs = sorted({c[0] for c in calls})
    assert procs == list(range(len(procs)))
    return columns.OpColumns(f=np.array(f, np.uint8), a=np.array(a, np.int32), b=np.array(b, np.int32),
                             process=np.array([calls[i][0] for i in order], np.int32), inv_pos=np.array([inv[i] for i in order], np.uint32),
                             ret_pos=np.array([ret.get(i, 0xFFFFFFFF) for i in order], np.uint32), n_events=len(events), n_process=len(procs))


def planted():
    """Seven slots, ~380 completions (six chunks):
    * slot 0: one call open from the 15th completion to the ~285th (over four chunks) while slots 1 - 3 complete three calls a time unit: its
      cursor does not move; ten short calls after it;
    * slot 4: three calls, all complete within the first chunk: its cursor runs to the tail sentinel and stays there;
    * slot 5: no call until the fourth chunk;
    * slot 6: one call invoked in the third chunk that never completes (it keeps the slot to the end)."""
    calls = [(0, 5.05, 95.05)] + [(0, 96.05 + j, 96.65 + j) for j in range(10)]
    calls += [(s, j + 0.25 * s, j + 0.25 * s + 0.6) for s in (1, 2, 3) for j in range(120)]
    calls += [(4, 0.11, 0.31), (4, 0.41, 0.61), (4, 0.71, 0.91)]
    calls += [(5, 70.07 + 2 * j, 71.07 + 2 * j) for j in range(5)]
    calls += [(6, 50.03, None)]
    h = by_hand(calls)
    assert h.n_process == 7 and 320 < int((h.ret_pos != 0xFFFFFFFF).sum()) <= 384
    return h


def ragged():
    """the ragged cases of tests/test_walk_emu.py, both seeds: a 1-op history, 64 and 65 ops, crashed calls that keep a slot to the end"""
    from test_walk_emu import SHAPES
    hs = [gen(n, p, busy, info=info, seed=s, corrupt=corrupt) for (n, p, busy, info, corrupt) in SHAPES for s in (1, 2)]
    assert all(h.n_process <= 64 for h in hs)
    return hs


def few_processes():
    """2 - 3 processes x 300 ops: more than four new calls of a slot in one chunk (the scan of invocation ranks takes several trips)"""
    return [gen(300, 2, 1.0, seed=1), gen(300, 3, 0.7, seed=2), gen(300, 3, 1.0, seed=3)]


def all_busy():
    """64 processes at busy 1.0, two values and five"""
    hs = [gen(400, 64, 1.0, seed=1, n_values=2), gen(400, 64, 1.0, seed=2, n_values=5)]
    assert all(56 <= h.n_process <= 64 for h in hs), [h.n_process for h in hs]
    return hs


def chunk_counts(run):
    """histories of 1, run - 1, run, run + 1 and 2 run + 1 chunks in one batch; the one of `run` chunks has a multiple of 64 completions"""
    fronts = sorted({30, 64 * (run - 1) - 10, 64 * run, 64 * run + 1, 64 * (2 * run + 1) - 30})
    hs = [_with_fronts(n, seed=10 + i) for i, n in enumerate(fronts)]
    assert {(n + 63) // 64 for n in fronts} == {1, run - 1, run, run + 1, 2 * run + 1}
    return hs


def _with_fronts(n_ret, seed):
    """a generated history with exactly n_ret completed calls (the generator drops the calls that fail)"""
    for n in range(n_ret, 2 * n_ret + 64):
        h = gen(n, 16, 0.4, seed=seed)
        if int((h.ret_pos != 0xFFFFFFFF).sum()) == n_ret:
            return h
    raise AssertionError(n_ret)


def small_shapes(run):
    return ragged() + few_processes() + all_busy() + [planted()] + chunk_counts(run)

"""Curated histories that take the count form's pipeline (csrc/batch_run.hip: count_form_pipeline, budgeted_pass, the relaxed sweep beside
first_pass) PAST ITS BUDGET of 32 probes per op on their own, one arm of oracle/wgl.py check_count_pipeline per line
(tests/test_count_form_arms_oracle.py pins the table on the CPU, tests/test_count_form_arms_gpu.py runs it on the device).

A history is columns.pair_events(synth.register_events(**gen)) with the reads listed in `stale` overwritten by a stale-but-plausible value
(op index, value).  A line names the ARM it is meant to reach and the SCHEDULE it reaches it under: width, round_pairs (the narrow kernel
at lanes_per_history = L is the oracle's width 1 at L pairs a round) and whether the relaxed level sweep runs in front; a line's budget
is the history's own, 32 probes per op (the mixed batches below name theirs: that of their longest member).  A line of the sweep route
names no width to the library; the one written here is what the library then takes for the history alone (default_width()).
`swept_valid` marks the lines of "exact, no budget" that get there because the relaxed sweep found the history valid under the relaxation.

All of them were picked from what scripts/count_form_arm_hunt.py prints: the smallest found for each arm that oracle.check(..., "window")
decides in a few million steps.  Every one has a crashed :write or :cas: a batch without any is no count-form batch (csrc/batch_create.hip,
plan_count_form) and takes none of these passes."""
from collections import namedtuple

import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns, synth

CAS = {"kind": 1, "init": N.NIL}
PROBE_CAP = 300_000          # every case's counters summed over its passes stay at or below this in the oracle

History = namedtuple("History", "gen stale")
Case = namedtuple("Case", "arm valid hist width round_pairs sweep swept_valid", defaults=(4, 64, False, False))


def _g(n_ops, n_procs, seed, busy, info, corrupt, n_values=5):
    return dict(n_ops=n_ops, n_procs=n_procs, seed=seed, busy=busy, info=info, corrupt=corrupt, n_values=n_values)


HISTORIES = {
    # linearizable, but the exact search overruns 32 probes per op
    "valid-a": History(_g(40, 16, 4002980, 1.0, 0.08, 0), [(11, 3)]),
    "valid-b": History(_g(40, 24, 7003964, 0.9, 0.3, 0), [(26, 0)]),
    "valid-c": History(_g(40, 24, 7002475, 0.9, 0.3, 0), [(15, 3)]),
    "valid-d": History(_g(100, 24, 697802, 1.0, 0.08, 0), [(55, 3), (46, 4)]),
    "valid-e": History(_g(200, 24, 628878, 1.0, 0.03, 0), []),
    "valid-f": History(_g(100, 16, 8023691, 0.9, 0.08, 0, 3), [(35, 2)]),
    # a stale read the relaxation accepts (a crashed :write of the value exists) and the exact counts refuse
    "stale-a": History(_g(100, 12, 8006850, 1.0, 0.08, 0), [(65, 4)]),
    "stale-b": History(_g(60, 16, 3003534, 0.6, 0.15, 0), [(47, 1), (40, 0)]),          # (its visited set outgrows 64 entries per op)
    "stale-c": History(_g(60, 16, 8022524, 1.0, 0.08, 0), [(37, 2), (39, 0)]),
    "stale-d": History(_g(60, 12, 8011561, 1.0, 0.15, 0), [(47, 4)]),
    # the relaxed search refutes at completion t, the prefix of t completions is linearizable
    "prefix-a": History(_g(40, 24, 4002499, 0.3, 0.15, 0.5, 3), [(7, 1)]),
    "prefix-b": History(_g(40, 16, 5001465, 1.0, 0.3, 0.5, 3), [(28, 1)]),
    "prefix-c": History(_g(40, 12, 1002830, 0.9, 0.3, 0.9, 3), [(5, 1)]),
    "prefix-d": History(_g(100, 16, 6004643, 1.0, 0.03, 0.9, 3), []),
    "prefix-e": History(_g(100, 24, 2002637, 0.3, 0.03, 0.9), [(30, 2)]),
    # ... the prefix is not: its own exhaustion names an earlier completion
    "exhausted-a": History(_g(500, 12, 6001225, 0.9, 0.03, 0.9), [(130, 0), (360, 4)]),
    "exhausted-b": History(_g(300, 24, 4000474, 0.6, 0.03, 0.9), [(66, 4), (71, 1)]),      # (a visited set of 75,058 configs: 335 per op)
    # refuted at the very first completion, after a blown budget (the only such history the hunt turned up)
    "first-a": History(_g(40, 24, 8009846, 0.9, 0.08, 0), [(2, 3), (26, 2)]),
    # the sweep route's small ones
    "sweep-first-a": History(_g(40, 6, 1000108, 0.9, 0.03, 0.9), [(23, 3), (2, 3)]),
    "sweep-first-b": History(_g(100, 16, 1000453, 0.3, 0.03, 0), [(1, 0), (68, 0)]),
    "sweep-first-c": History(_g(100, 8, 718368, 1.0, 0.15, 0.5), [(11, 4), (5, 4)]),
    "sweep-exhausted-a": History(_g(40, 6, 1001316, 0.9, 0.3, 0.9), [(11, 1), (3, 1)]),
    "sweep-exhausted-b": History(_g(60, 8, 1000234, 1.0, 0.3, 0.5), [(7, 0), (36, 3)]),
    "sweep-exhausted-c": History(_g(60, 6, 4001242, 0.3, 0.15, 0.9, 3), [(1, 2), (29, 0)]),
    # the degenerate two
    "all-crashed": History(_g(12, 4, 31, 0.5, 1.0, 0), []),
    "calm": History(_g(300, 8, 5000, 0.3, 0.05, 0), []),
}

# Lines whose visited set outgrows, within ONE pass after the budget, the first size budgeted_pass gives it (64 entries per op, rounded up to a
# power of two) -- the pass is taken again with a set 16 times the size: (history, width, sweep route) -> the first pass that outgrows it.
# exhausted-b outgrows it in the RELAXED pass (no targets); its prefix pass inherits the larger set.  NO line outgrows it in a pass that
# carries a prefix target: budgeted_pass's second round with targets (`atg`) stays uncrossed on the device.
REGROWN = {("stale-b", 4, False): "exact, no budget", ("exhausted-b", 4, False): "relaxed"}
# The one candidate for it is exhausted-b on the sweep route: the oracle's relaxed sweep refutes it and its single (targeted) prefix pass
# visits 19,367 configs against a first size of 16,384.  On the device the relaxed sweep does not conclude for this history -- its bursts
# outgrow the sweep's sets (the oracle's sweep holds 4,238 configs pending at once; the kernel's largest sets hold 2,048) -- which proves
# nothing, and the library takes the depth-first passes instead (csrc/batch_run.hip, count_form_pipeline: pend_dfs).
# check_count_pipeline(relaxed_sweep=True) does not state a sweep that gives up; what tbc_check answers is the pipeline WITHOUT the sweep.
SWEEP_GIVES_UP = ("exhausted-b",)
SWEEP_SET_SIZE = 2048          # csrc/tbc_internal.h kSweepCapBig


def first_table_size(ops):
    return 1 << int(np.ceil(np.log2(64 * max(len(ops), 1))))


_BUILT = {}


def history(name_or_hist):
    """the OpColumns of a named history (built once, never written to afterwards)"""
    h = HISTORIES[name_or_hist] if isinstance(name_or_hist, str) else name_or_hist
    key = (tuple(sorted(h.gen.items())), tuple(h.stale))
    if key not in _BUILT:
        ops = columns.pair_events(synth.register_events(**h.gen))
        for i, v in h.stale:
            assert ops.f[i] == N.F_READ and ops.ret_pos[i] != N.POS_CRASHED and ops.a[i] != N.NIL, (h, i)
            ops.a[i] = v
        _BUILT[key] = ops
    return _BUILT[key]


def default_width(hists):
    """The width the library takes when none is named (csrc/batch_create.hip): 4, and 2 where at most 10 calls are in flight on average --
    the positions from invocation to completion over the events, a crashed call (in the count form: no open call) left out."""
    open_sum = events = 0
    for h in hists:
        inv, ret = np.asarray(h.inv_pos).astype(np.int64), np.asarray(h.ret_pos).astype(np.int64)
        live = ret != N.POS_CRASHED
        open_sum += int((ret[live] - inv[live]).sum())
        events += h.n_events
    return 2 if events and open_sum <= 10 * events else 4


_W2, _W16, _N8, _N16 = dict(width=2), dict(width=16), dict(width=1, round_pairs=8), dict(width=1, round_pairs=16)


def _c(arm, valid, hist, **kw):
    return Case(arm, valid, hist, **kw)


def _s(arm, valid, hist, width=2, swept_valid=False):
    """a line of the sweep route; width: what the library takes for the history alone (2 at ten calls in flight or fewer, else 4)"""
    return Case(arm, valid, hist, width=width, sweep=True, swept_valid=swept_valid)


CASES = [
    # ---- depth-first route (search_width / lanes_per_history named: no sweep)
    _c("exact, no budget", 1, "valid-a"), _c("exact, no budget", 1, "valid-b"), _c("exact, no budget", 1, "valid-c"),
    _c("exact, no budget", 1, "valid-a", **_W16), _c("exact, no budget", 1, "valid-b", **_W2), _c("exact, no budget", 1, "valid-b", **_N8), _c("exact, no budget", 1, "valid-c", **_N16),
    _c("exact, no budget", 0, "stale-a"), _c("exact, no budget", 0, "stale-b"),
    _c("exact, no budget", 0, "stale-a", **_W16), _c("exact, no budget", 0, "stale-b", **_W2), _c("exact, no budget", 0, "stale-a", **_N8), _c("exact, no budget", 0, "stale-b", **_N16),
    _c("prefix", 0, "prefix-a"), _c("prefix", 0, "prefix-b"), _c("prefix", 0, "prefix-c"),
    _c("prefix", 0, "prefix-a", **_W16), _c("prefix", 0, "prefix-b", **_W2), _c("prefix", 0, "prefix-b", **_N8), _c("prefix", 0, "prefix-c", **_N16),
    _c("prefix exhausted", 0, "exhausted-a"), _c("prefix exhausted", 0, "exhausted-b"),
    _c("prefix exhausted", 0, "exhausted-a", **_W16), _c("prefix exhausted", 0, "exhausted-a", **_W2), _c("prefix exhausted", 0, "exhausted-a", **_N8), _c("prefix exhausted", 0, "exhausted-a", **_N16),
    _c("relaxed", 0, "first-a"), _c("relaxed", 0, "first-a", **_W2), _c("relaxed", 0, "first-a", **_N8), _c("relaxed", 0, "first-a", **_N16),
    # ---- sweep route (tbc_check with the library's defaults: the relaxed level sweep beside the exact search, the width the library's)
    _s("relaxed sweep", 0, "sweep-first-a"), _s("relaxed sweep", 0, "sweep-first-b"), _s("relaxed sweep", 0, "sweep-first-c"), _s("relaxed sweep", 0, "first-a"),
    _s("relaxed sweep, prefix", 0, "prefix-a"), _s("relaxed sweep, prefix", 0, "prefix-b"),
    _s("relaxed sweep, prefix exhausted", 0, "sweep-exhausted-a"), _s("relaxed sweep, prefix exhausted", 0, "sweep-exhausted-b"),
    _s("relaxed sweep, prefix exhausted", 0, "sweep-exhausted-c"), _s("relaxed sweep, prefix exhausted", 0, "exhausted-a"),
    _s("exact, no budget", 1, "valid-c", 2, True), _s("exact, no budget", 1, "valid-b", 4, True),
    _s("exact, no budget", 0, "stale-a", 2, True), _s("exact, no budget", 0, "stale-b", 2, True),
    _s("exact", 1, "all-crashed"), _s("exact", 1, "calm"),
]

# at least this many lines per (arm, verdict, route) for the wide kernel at width 4 / another width / the narrow kernel
DFS_ARMS = (("exact, no budget", 1), ("exact, no budget", 0), ("prefix", 0), ("prefix exhausted", 0))
SWEEP_ARMS = (("relaxed sweep", 0, False), ("relaxed sweep, prefix", 0, False), ("relaxed sweep, prefix exhausted", 0, False),
              ("exact, no budget", 1, True), ("exact, no budget", 0, True))

# ---- the mixed batches.  The depth-first one: two or more of every depth-first arm UNDER THE BUDGET OF ITS LONGEST MEMBER (exhausted-a, 367
# ops: 11,744 probes -- the small cases above end inside that and are its "exact" members), the arms alternating
MIXED_DFS = ("valid-d", "stale-c", "prefix-d", "exhausted-a", "calm", "valid-e", "stale-d", "prefix-e", "exhausted-b", "valid-a", "valid-f", "first-a")
MIXED_SWEEP = ("sweep-first-a", "prefix-b", "sweep-exhausted-b", "valid-f", "all-crashed", "calm", "exhausted-a", "stale-c")
# histories that all end "exact": what a count-form batch is created from before the mixed set is sent to it as a fresh input
CALM = [History(_g(380 + 3 * s, 8, 6100 + s, 0.3, 0.05, 0.5 if s % 3 == 0 else 0), []) for s in range(len(MIXED_DFS))]

_PIPE, _PASSES = {}, {}


def pipeline(oracle, hist, width=4, round_pairs=64, sweep=False, longest=None, want_witness=False):
    """oracle.check_count_pipeline of a history under a schedule (longest: the longest history of the batch it stands in, None: alone),
    computed once -> (valid, fail_op, last pass, sums, arm)"""
    ops = history(hist)
    budget = 32 * (len(ops) if longest is None else longest)
    key = (id(ops), width, round_pairs, sweep, budget, want_witness)
    if key not in _PIPE:
        seen = []
        e = oracle.check_count_pipeline(ops.as_dict(), CAS, width=width, budget=budget, want_witness=want_witness, round_pairs=round_pairs, relaxed_sweep=sweep,
                                        on_pass=lambda name, r: seen.append((name, r["visited"])))
        assert e is not None, hist
        _PIPE[key], _PASSES[key] = e, seen
    return _PIPE[key]


def passes(oracle, hist, width=4, round_pairs=64, sweep=False):
    """[(pass, configs in its visited set)] of the depth-first passes the pipeline runs for the history alone, in order"""
    pipeline(oracle, hist, width, round_pairs, sweep)
    ops = history(hist)
    return _PASSES[(id(ops), width, round_pairs, sweep, 32 * len(ops), False)]


def case_pipeline(oracle, c, want_witness=False):
    return pipeline(oracle, c.hist, c.width, c.round_pairs, c.sweep, None, want_witness)


def prev_op(ops, fail_op):
    """the op whose completion rank is one below fail_op's (None at rank 0), from ret_pos alone"""
    ret = np.asarray(ops.ret_pos).astype(np.int64)
    earlier = np.flatnonzero(ret < ret[fail_op])
    return None if len(earlier) == 0 else int(earlier[np.argmax(ret[earlier])])


def expected(oracle, hist, width=4, round_pairs=64, sweep=False, longest=None, want_witness=False):
    """what the device must return for a history under a schedule, as a dict: valid, fail_op, prev (of an INVALID answer), final_state, the
    counters summed over the passes, the arm, and `prefix_state`: the final state of the oracle's prefix pass where the arm ends in one"""
    v, fo, last, tot, arm = pipeline(oracle, hist, width, round_pairs, sweep, longest, want_witness)
    ops = history(hist)
    return {"valid": v, "fail_op": fo if v == 0 else None, "prev": prev_op(ops, fo) if v == 0 else None, "final_state": last["final_state"],
            "probes": tot["probes"], "visited": tot["visited"], "backtracks": tot["expanded"], "arm": arm,
            "witness": last.get("witness"), "prefix_state": last["final_state"] if arm.endswith("prefix") else None}


def arms_of(oracle, names, width=4, round_pairs=64, sweep=False):
    """{arm, verdict: how many} of a batch of named histories under the budget of its longest (sweep route: at the library's width for it)"""
    if sweep:
        width = default_width([history(n) for n in names])
    longest = max(len(history(n)) for n in names)
    out = {}
    for n in names:
        v, _, _, _, arm = pipeline(oracle, n, width, round_pairs, sweep, longest)
        out[(arm, v)] = out.get((arm, v), 0) + 1
    return out

"""Histories, batch sizes and references for the tests of the batch-size classes (tests/test_batch_sizes_oracle.py on the CPU,
tests/test_batch_sizes_gpu.py on the device).

The number of histories in a batch decides which pack kernel runs (<= 8: pack_one; 9 .. 64: pack_wg / pack_wg64, the lists sized on the
host, 1,024 threads a block; >= 65: the lists sized on the device, 256 threads a block), how stream_assign_lists_kernel deals the lists'
places (>= 1,025: several histories a thread) and how often the grid loops of pack_kernel / open_counts_kernel / open_dprod_kernel /
count_fronts_kernel go round (>= 4,097: more than once).  A history's answer must not depend on any of it.

Every FAMILY is 61 distinct seeded histories (61 is prime: a history's position relative to 64, 1,024 and 4,096 shifts from copy to
copy), of lengths that never align, every third with a planted bad read, and names its SCHEDULE in make_opts -- so the library's
size-dependent choices (a level sweep for few histories, the width, the lanes) are out of the way and ONE reference per base history
serves every batch size."""
from collections import namedtuple

import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns, core, synth

CAS = {"kind": 1, "init": N.NIL}
N_BASE = 61
SIZES = (1, 8, 9, 64, 65, 256, 257, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8200)      # (8,200: two full trips of the grid loops and a partial third)
FEW_SIZES = (8, 9, 64, 65, 4095, 4097)
LONG_SIZES = (9, 65, 4097)
EDGES = (64, 1024, 4096)
CRASHED = 0xFFFFFFFF
OTHER_SEEDS = 600          # other_base(): the same shapes from seeds this far away (every crashed family keeps its minimum of crashed calls there)

# kind: "narrow" (several histories per wavefront, oracle/wgl_beam.c at one config and eight pairs a round), "wide" (wgl_beam.c at four
# configs a round), "count" (oracle/wgl_count.c, the library's passes); words: the mask words the batch's widest history asks for
Family = namedtuple("Family", "gen seed0 kind opts words vmax min_crashed order long_neighbour", defaults=(0, 0, False))

_NARROW = dict(lanes_per_history=8, count_form=False)
_WIDE = dict(search_width=4, order_restarts=False, count_form=False)
_G16 = dict(n=120, p=16, busy=0.2)
_G16W = dict(n=120, p=16, busy=0.3)
_G70 = dict(n=260, p=70, busy=0.08)
_G150 = dict(n=520, p=150, busy=0.04)
# (the planted bad read holds n_values + 7: 12 in the families of values 0 .. 4 -- rows of 16 entries, open_walk_fronts_kernel<32> --,
# exactly 30 with values 0 .. 22 -- full rows of 32 --, 47 with values 0 .. 39: no rule tables)
_V30 = dict(n=150, p=12, busy=0.3, n_values=23)
_V40 = dict(n=150, p=12, busy=0.3, n_values=40)

FAMILIES = {
    "narrow-1w": Family(_G16, 11000, "narrow", _NARROW, 1, 12),
    "narrow-1w-shipped-order": Family(_G16, 11000, "narrow", dict(_NARROW, list_order=N.ORDER_DEFAULT), 1, 12, order=16 + 24),
    "wide-1w": Family(_G16W, 12000, "wide", _WIDE, 1, 12),
    "wide-2w": Family(_G70, 13000, "wide", _WIDE, 2, 12),
    "wide-4w": Family(_G150, 14000, "wide", _WIDE, 4, 12),
    "narrow-2w": Family(_G70, 13000, "narrow", _NARROW, 2, 12),
    "values-to-30-wide": Family(_V30, 15000, "wide", _WIDE, 1, 30),
    "values-to-30-narrow": Family(_V30, 15000, "narrow", _NARROW, 1, 30),
    "values-past-30-wide": Family(_V40, 16000, "wide", _WIDE, 1, 47),
    "crashed-mask-wide": Family(dict(n=150, p=8, busy=0.3, info=0.03), 17000, "wide", _WIDE, 1, 12, min_crashed=2),
    "count-wide": Family(dict(n=150, p=8, busy=0.3, info=0.06), 18000, "count", dict(search_width=4, count_form=True), 1, 12, min_crashed=5),
    "count-narrow": Family(dict(n=150, p=8, busy=0.3, info=0.06), 18000, "count", dict(lanes_per_history=8, count_form=True), 1, 12, min_crashed=5),
    "long-neighbour-wide": Family(_G16W, 12000, "wide", _WIDE, 1, 12, long_neighbour=True),
    "long-neighbour-narrow": Family(_G16, 11000, "narrow", _NARROW, 1, 12, long_neighbour=True),
    # the two inputs of the arena-overflow test alone (OVERFLOW_N histories each)
    "quiet-narrow": Family(dict(n=123, p=16, busy=0.05), 19000, "narrow", _NARROW, 1, 12),
    "dense-narrow": Family(dict(n=120, p=16, busy=0.6), 20000, "narrow", _NARROW, 1, 12),
}
OVERFLOW_FAMILIES = ("quiet-narrow", "dense-narrow")
OVERFLOW_N = 1500                      # stream_assign_lists_kernel: per = ceil(1500 / 1024) = 2 histories a thread
SIZE_FAMILIES = tuple(n for n in FAMILIES if n not in OVERFLOW_FAMILIES)          # created at the size classes ...
ALL_SIZES_FAMILIES = ("narrow-1w", "wide-1w", "wide-2w", "count-wide")            # ... these at every one of SIZES
STREAM_FAMILIES = SIZE_FAMILIES        # ... and sent fresh inputs: csrc/batch_stream.hip's streamable() lets every one of them through
RELOAD_PAIRS = ((9, 1), (65, 64), (1025, 9), (1025, 1024), (2049, 2049), (4097, 1025), (4097, 4097))          # (created, reloaded), ascending

# what one history may be for a batch to keep pack_wg_kernel (csrc/pack_one_impl.h, BatchGeo)
GEO_OPS, GEO_EVENTS, GEO_SLOTS = 8192, 32768, 256


def gen(n, p, busy, seed, info=0.0, corrupt=0.0, **kw):
    return columns.pair_events(synth.register_events(n_ops=n, n_procs=p, seed=seed, busy=busy, info=info, corrupt=corrupt, **kw))


def _family_history(fam, s, seed0=None):
    g = dict(fam.gen)
    n = g.pop("n") + 7 * (s % 9)
    return gen(n, g.pop("p"), g.pop("busy"), (fam.seed0 if seed0 is None else seed0) + s, corrupt=0.5 if s % 3 == 0 else 0.0, **g)


_BASE, _LONG = {}, {}
_REFS, _LONG_REFS, _SHAPE_CHECKED = {}, {}, set()          # (family, which, history, budget) -> reference; kind -> the long neighbour's; (family, which)


def base(name):
    """the family's 61 base histories"""
    fam = FAMILIES[name]
    key = (tuple(sorted(fam.gen.items())), fam.seed0)
    if key not in _BASE:
        _BASE[key] = [_family_history(fam, s) for s in range(N_BASE)]
    return _BASE[key]


def other_base(name):
    """61 histories of the same shape from other seeds: what a reload swaps in for a third of the histories"""
    fam = FAMILIES[name]
    key = (tuple(sorted(fam.gen.items())), fam.seed0 + OTHER_SEEDS)
    if key not in _BASE:
        _BASE[key] = [_family_history(fam, s, fam.seed0 + OTHER_SEEDS) for s in range(N_BASE)]
    return _BASE[key]


def long_neighbour():
    """one history too long for the workgroup pack's LDS tables: with it in the batch, every history is packed by pack_kernel"""
    if "h" not in _LONG:
        _LONG["h"] = gen(12000, 16, 0.1, 424242)
    return _LONG["h"]


def make_opts(name, **kw):
    return core.make_opts(time_limit_ms=120000, algorithm=N.ALG_COMPETITION, want_witness=False, **dict(FAMILIES[name].opts, **kw))


def budget_of(batch):
    """the count form's budget of probes for its first pass: 32 per op of the batch's longest history"""
    return 32 * max(len(h) for h in batch)


def reference(oracle, name, h, budget=None):
    """The oracle's statement of the family's schedule for one history, as a dict of what the device must return:
    valid, fail_op, final_state (of a valid history: the state the linearization found ends in; the count form's is its last pass's) and
    the counters probes, visited, backtracks and (not the count form: its passes' deepest stacks are not summed) max_depth."""
    fam = FAMILIES[name]
    d = h.as_dict()
    if fam.kind == "count":
        narrow = "lanes_per_history" in fam.opts
        e = oracle.check_count_pipeline(d, CAS, width=1 if narrow else 4, budget=budget, round_pairs=8 if narrow else 64)
        assert e is not None
        v, fo, last, tot, how = e
        return {"valid": v, "fail_op": fo, "final_state": last["final_state"], "probes": tot["probes"], "visited": tot["visited"], "backtracks": tot["expanded"], "how": how}
    if fam.kind == "narrow":
        e = oracle.check_beam(d, CAS, 1, round_pairs=8, rules_at_any_round_size=True, branch_lists=True, want_witness=False,
                              list_order=oracle.ORACLE_LIST_ORDER[fam.order])
    else:
        e = oracle.check_beam(d, CAS, 4, want_witness=False)
    return {"valid": e["valid"], "fail_op": e["fail_op"], "final_state": e["final_state"], "probes": e["probes"], "visited": e["visited"],
            "backtracks": e["expanded"], "max_depth": e["max_stack"]}


def _values(h):
    f, a, b = np.asarray(h.f), np.asarray(h.a, np.int64), np.asarray(h.b, np.int64)
    v = np.concatenate([a, b[f == N.F_CAS]])
    return v[v != N.NIL]


def mask_words(hists):
    """1, 2 or 4 (3 takes the kernels of 4): the 64-bit words that hold a bit per process slot of the batch's widest history"""
    w = (max(h.n_process for h in hists) + 63) // 64
    return 4 if w == 3 else w


def largest_value(hists):
    return max(int(_values(h).max()) for h in hists)


def check_shape(oracle, name, hists):
    """the family has the shape it is named for"""
    fam = FAMILIES[name]
    assert mask_words(hists) == fam.words, (name, max(h.n_process for h in hists))
    assert largest_value(hists) == fam.vmax, name
    n_crashed = [int((np.asarray(h.ret_pos) == CRASHED).sum()) for h in hists]
    assert min(n_crashed) >= fam.min_crashed, (name, min(n_crashed))
    if not fam.min_crashed:
        assert max(n_crashed) == 0, name
    for h in hists:
        assert len(h) <= GEO_OPS and h.n_events <= GEO_EVENTS and h.n_process <= GEO_SLOTS, name
    if fam.kind == "count":
        narrow = "lanes_per_history" in fam.opts
        for i, h in enumerate(hists):
            assert oracle.check_count(h.as_dict(), CAS, width=1 if narrow else 4, max_probes=1, round_pairs=8 if narrow else 64, want_witness=False) is not None, (name, i)
    if fam.long_neighbour:
        assert len(long_neighbour()) > GEO_OPS and long_neighbour().n_process <= 64


def _ref(oracle, name, which, j, budget=None):
    """reference() of history j of base(name) / other_base(name), computed once (the count form's: once per budget)"""
    key = (name, which, j, budget)
    if key not in _REFS:
        _REFS[key] = reference(oracle, name, (base(name) if which == "base" else other_base(name))[j], budget)
    return _REFS[key]


def references(oracle, name, which="base"):
    """Each base history's reference (the count form's under the budget the whole family makes; expected() asks again for a batch
    whose longest history makes another).  First: the family has the shape it is named for; then: the oracle decides every history,
    and at least 15 of the 61 are invalid."""
    hists = base(name) if which == "base" else other_base(name)
    fam = FAMILIES[name]
    if (name, which) not in _SHAPE_CHECKED:
        check_shape(oracle, name, hists)
        _SHAPE_CHECKED.add((name, which))
    budget = budget_of(hists) if fam.kind == "count" else None
    refs = [_ref(oracle, name, which, j, budget) for j in range(N_BASE)]
    verdicts = [r["valid"] for r in refs]
    assert set(verdicts) <= {0, 1}, (name, verdicts)
    assert verdicts.count(0) >= 15 and verdicts.count(1) >= 15, (name, verdicts.count(0))
    if fam.long_neighbour:
        assert long_reference(oracle, name)["valid"] == 1
    return refs


def long_reference(oracle, name):
    kind = FAMILIES[name].kind
    if kind not in _LONG_REFS:
        _LONG_REFS[kind] = reference(oracle, name, long_neighbour())
    return _LONG_REFS[kind]


def indices(n, rot=None):
    """which base history stands at each place of a batch of n: the rotation depends on n, so that every class sees other neighbours"""
    rot = 7 * n if rot is None else rot
    return [(i + rot) % N_BASE for i in range(n)]


def batch_of(name, n, long_at=None, rot=None):
    """[base[(i + 7 n) % 61] for i in range(n)]; a long-neighbour family has its long history at place n // 2 (or long_at) in the place
    of the base history there"""
    b = base(name)
    out = [b[j] for j in indices(n, rot)]
    if FAMILIES[name].long_neighbour:
        out[n // 2 if long_at is None else long_at] = long_neighbour()
    return out


def expected(oracle, name, batch, idx, which=None):
    """the references of a batch whose place i holds base history idx[i] (other_base's where which[i]); the long neighbour is
    recognised by identity"""
    fam = FAMILIES[name]
    references(oracle, name)
    if which is not None and any(which):
        references(oracle, name, "other")
    budget = budget_of(batch) if fam.kind == "count" else None
    out = []
    for i, (h, j) in enumerate(zip(batch, idx)):
        if fam.long_neighbour and h is long_neighbour():
            out.append(long_reference(oracle, name))
        else:
            out.append(_ref(oracle, name, "other" if which is not None and which[i] else "base", j, budget))
    return out


def reload_arrangement(name, n, rot, t_mod4=None):
    """Another arrangement of the family for a fresh input: another rotation, every third place a history from other seeds, a
    long-neighbour family's long history at place n // 2, and (where t_mod4 is given) the last place the first base history that makes
    the input's total ops = t_mod4 (mod 4); an input of the long history alone has the total it has.
    -> (histories, base indices, which places hold other seeds)"""
    idx = indices(n, rot)
    which = [i % 3 == 1 for i in range(n)]
    b, o = base(name), other_base(name)
    hists = [o[j] if w else b[j] for j, w in zip(idx, which)]
    if FAMILIES[name].long_neighbour:
        hists[n // 2] = long_neighbour()
    if t_mod4 is not None and hists[-1] is not long_neighbour():
        rest = sum(len(h) for h in hists[:-1])
        j = next(j for j in range(N_BASE) if (rest + len(b[j])) % 4 == t_mod4)
        hists[-1], idx[-1], which[-1] = b[j], j, False
    return hists, idx, which


# ---- lists that outgrow the arena behind 1,024 histories (csrc/batch_stream.hip, stream_assign_lists_kernel)


def list_entries(h, branch_lists=True):
    """Entries of a history's per-front lists, as csrc/batch_create.hip's open_list_entries counts them: every live call once per front it is
    open at -- the completions between its invocation and its own, and its own; branch lists (the narrow kernel under the eager-read
    rule) hold no reads.  At least 1."""
    inv, ret, f = np.asarray(h.inv_pos, np.int64), np.asarray(h.ret_pos, np.int64), np.asarray(h.f)
    live = ret != CRASHED
    done = np.sort(ret[live])
    listed = live & ~((f == N.F_READ) & branch_lists)
    total = int((np.searchsorted(done, ret[listed]) - np.searchsorted(done, inv[listed]) + 1).sum())
    return max(1, total)


def fallback_start(first, nxt):
    """The first history of `nxt` whose lists end beyond the arena of a narrow batch created from `first` (more than 64 histories: the
    arena is what the first input's lists take; the first fresh input finds it a sixteenth and 4,096 entries larger) -- len(nxt) where
    everything fits.  The running sum only grows: every history from there on falls back.
    The headroom is csrc/batch_stream.hip's, stream_consume(), where a batch meets its first fresh input (`B->d_lst.n + B->d_lst.n / 16 +
    4096`): a retune there moves the place this predicts, and the constant here with it."""
    have = sum(list_entries(h) for h in first)
    cap = have + have // 16 + 4096
    ends = np.cumsum([list_entries(h) for h in nxt])
    return int(np.searchsorted(ends, cap, side="right"))


def overflow_batches():
    """-> (1,500 quiet histories, 1,500 dense ones, the dense ones' base indices)"""
    n = OVERFLOW_N
    return batch_of("quiet-narrow", n), batch_of("dense-narrow", n), indices(n)


# ---- the wire format's edges (csrc/batch_stream.hip, stream_unpack_kernel: four ops a thread, the tail by single ops)
def sequential(calls):
    """one process, one call after the other: calls = (f, a, b)"""
    n = len(calls)
    return columns.OpColumns(f=np.array([c[0] for c in calls], np.uint8), a=np.array([c[1] for c in calls], np.int32), b=np.array([c[2] for c in calls], np.int32),
                             process=np.zeros(n, np.int32), inv_pos=np.arange(0, 2 * n, 2, dtype=np.uint32), ret_pos=np.arange(1, 2 * n, 2, dtype=np.uint32),
                             n_events=2 * n, n_process=1)


def renamed(h, top=254):
    """the history with every value v as top - v (nil stays nil): as linearizable as it was"""
    f, a, b = np.asarray(h.f), np.asarray(h.a), np.asarray(h.b)
    na = np.where(a == N.NIL, a, top - a).astype(np.int32)
    nb = np.where((f == N.F_CAS) & (b != N.NIL), top - b, b).astype(np.int32)
    return columns.OpColumns(f=f.copy(), a=na, b=nb, process=np.asarray(h.process).copy(), inv_pos=np.asarray(h.inv_pos).copy(), ret_pos=np.asarray(h.ret_pos).copy(),
                             n_events=h.n_events, n_process=h.n_process)


def wire_edge_input(n=65):
    """A fresh input for a values-past-30 batch: the family's histories with value v renamed 254 - v, so that 254 (the wire format's largest)
    stands in :write calls and in both arguments of :cas calls all over the four-op path, and as the LAST history three sequential calls
    -- a read of nil, a write of 254, a cas of 254 to 254 -- that are the scalar tail (the total is 3 mod 4)."""
    turned = [renamed(h) for h in base("values-past-30-wide")]
    hists = [turned[j] for j in indices(n - 1, 3)]
    rest = sum(len(h) for h in hists[:-1])
    hists[-1] = next(h for h in turned if (rest + len(h)) % 4 == 0)
    return hists + [sequential([(N.F_READ, N.NIL, 0), (N.F_WRITE, 254, 0), (N.F_CAS, 254, 254)])]


# ---- fresh inputs across the classes
def reload_cases():
    """(family, histories created, histories reloaded, the reloaded input's total ops mod 4), by size ascending; the totals go through
    0, 1, 2, 3 in turn, so that stream_unpack_kernel's scalar tail is 0, 1, 2 and 3 ops long (the long neighbour reloaded alone has its own)"""
    alone = len(long_neighbour()) % 4
    return [(name, nc, nr, alone if FAMILIES[name].long_neighbour and nr == 1 else (k + i) % 4)
            for k, (nc, nr) in enumerate(RELOAD_PAIRS) for i, name in enumerate(STREAM_FAMILIES)]


def reload_plan(name, n_create, n_reload, t_mod4):
    """-> (the histories the batch is created from, their base indices, (the reloaded histories, base indices, which are from other seeds))"""
    return batch_of(name, n_create), indices(n_create), reload_arrangement(name, n_reload, rot=3 * n_create + 11, t_mod4=t_mod4)

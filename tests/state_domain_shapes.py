"""Histories, models and classes for the tests of the STATE WORD's edges -- the model's initial value and the value-domain classes
(tests/test_state_domain_oracle.py and tests/test_state_domain_emu.py on the CPU, tests/test_state_domain_gpu.py on the device).

csrc/batch_create.hip, plan_engines: vmax = max(init, the largest value any op holds); with every value and the init >= 0 and vmax <= 30
(tbc_internal.h kMaxRuleValue) the batch has rule tables -- n_dom = vmax + 2 states (nil, 0 .. vmax), vpad = the next power of two -- and from
there follow the front record (compact 64 B only at n_dom <= 6 and one mask word: front_compact_ok), the walk kernel (open_walk_fronts_kernel<8>
at vpad <= 8, else <32>: pack_open.hip), front_stride(vpad, mask_words) and the sweep's cut_open (plan_sweep_segments: the largest m <= 4 with
n_dom << m <= 32 * TBC_SWEEP_SLICES = 128).  Anything else -- a value of 31, a negative value, a negative init -- switches tables, lookahead
records and the count form off.  An init above every op's value moves a batch into another class ON ITS OWN, so every class is built twice:

  by values   the ops hold 0 .. vmax, the init is nil
  by init     the ops write 0 .. vmax - 2 only and init = vmax (reads of the init are the point of it)

A case is about 12 histories of 8 / 40 / 200 / 600 ops, 3 .. 16 processes, busy 0.3 .. 0.8, a third of them invalid by a read of an IN-DOMAIN value
(nothing leaves the class); the crashed cases stop at 200 ops (every crashed call stays a candidate to the end: longer ones are the count form's
own tests').  Histories come from the C generator (include/tbsynth.h; it simulates from nil, so for a by-init case every completed read of nil is
relabelled a read of the init), from simulate() below (a register that STARTS at the init) and, per by-init case, from four hand shapes:
a :cas [init x] that succeeds before any write, a read of the init open across the first write, reads of the init and of nil alone (nothing to
search: final_state is the init), and a read of another in-domain value before any write (the one flaw of that history)."""
import functools
import heapq
import random
from collections import namedtuple

import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns, core, synth
from jepsen_tigerbeetle_amd.knossos import model as M, op as kop

NIL = N.NIL
CRASHED = 0xFFFFFFFF
MAX_RULE_VALUE = 30                       # tbc_internal.h kMaxRuleValue
SWEEP_ORIGINS = 32 * N.SWEEP_SLICES       # plan_sweep_segments: n_dom << cut_open <= 32 * kSweepSlices

Class = namedtuple("Class", "n_dom vpad rules compact walk cut_open")
NO_TABLES = Class(0, 0, False, False, None, 0)
# how: "values" / "init"; vmax: the case's largest value (by init: the init); kind: 1 cas-register, 0 register; procs: 0 = the mix's own
Case = namedtuple("Case", "name how vmax init lo kind info procs cls", defaults=(1, 0.0, 0, None))


def value_class(init, hists, mask_words=1):
    """csrc/batch_create.hip plan_engines / plan_sweep_segments, tbc_internal.h front_compact_ok, pack_open.hip's launch: restated"""
    vals = [values_of(h) for h in hists]
    vals = np.concatenate(vals) if vals else np.zeros(0, np.int64)
    vmax = max(-1 if init == NIL else init, int(vals.max()) if len(vals) else -1)
    in_range = (init == NIL or init >= 0) and (len(vals) == 0 or int(vals.min()) >= 0)
    if not in_range or vmax > MAX_RULE_VALUE:
        return NO_TABLES
    n_dom = vmax + 2
    vpad = 2
    while vpad < n_dom:
        vpad <<= 1
    cut = 0
    while cut < 4 and (n_dom << (cut + 1)) <= SWEEP_ORIGINS:
        cut += 1
    return Class(n_dom, vpad, True, mask_words == 1 and 2 <= n_dom <= 6, 8 if vpad <= 8 else 32, cut)


def front_stride(vpad, mask_words):
    """tbc_internal.h front_stride(): u64 words of a plain front record"""
    return (vpad * mask_words + 6 + 7) & ~7


def _cls(n_dom, words=1):
    """the class a case is NAMED for, written out (tests/test_state_domain_oracle.py holds value_class() of its histories against it, the device
    test tbc_batch_sweep_info): vpad the next power of two, the compact record up to n_dom 6, the <8> walk up to vpad 8, and cut_open by
    plan_sweep_segments' loop (n_dom << m <= 128, m <= 4): 4 up to n_dom 8, 3 up to 16, 2 up to 32."""
    vpad = 2
    while vpad < n_dom:
        vpad <<= 1
    return Class(n_dom, vpad, True, words == 1 and n_dom <= 6, 8 if vpad <= 8 else 32, 4 if n_dom <= 8 else 3 if n_dom <= 16 else 2)


DOMS = (2, 4, 5, 6, 7, 8, 9, 16, 17, 32)
CRASHED_DOMS = (6, 8, 32)


def _cases():
    out = []
    for d in DOMS:
        out.append(Case(f"dom{d}-values", "values", d - 2, NIL, 0, cls=_cls(d)))
        out.append(Case(f"dom{d}-init", "init", d - 2, d - 2, 0, cls=_cls(d)))
    out.append(Case("vmax31-values", "values", 31, NIL, 0, cls=NO_TABLES))
    out.append(Case("init31", "init", 31, 31, 0, cls=NO_TABLES))
    out.append(Case("negative-value", "values", 2, NIL, -2, cls=NO_TABLES))          # the ops hold -2 .. 2
    out.append(Case("negative-init", "init", 3, -1, 0, cls=NO_TABLES))               # init -1, the ops 0 .. 3
    for d in (6, 8):
        out.append(Case(f"dom{d}-register", "values", d - 2, NIL, 0, kind=0, cls=_cls(d)))
    out.append(Case("dom16-2w-values", "values", 14, NIL, 0, procs=70, cls=_cls(16, 2)))
    out.append(Case("dom32-2w-init", "init", 30, 30, 0, procs=70, cls=_cls(32, 2)))
    for d in CRASHED_DOMS:
        out.append(Case(f"dom{d}-crashed-values", "values", d - 2, NIL, 0, info=0.1, cls=_cls(d)))
        out.append(Case(f"dom{d}-crashed-init", "init", d - 2, d - 2, 0, info=0.1, cls=_cls(d)))
    out.append(Case("vmax31-crashed-values", "values", 31, NIL, 0, info=0.1, cls=NO_TABLES))
    out.append(Case("init31-crashed", "init", 31, 31, 0, info=0.1, cls=NO_TABLES))
    return {c.name: c for c in out}


CASES = _cases()
NAMES = tuple(CASES)
BY_INIT = tuple(n for n, c in CASES.items() if c.how == "init")
CRASHED_CASES = tuple(n for n, c in CASES.items() if c.info)
TWO_WORDS = tuple(n for n, c in CASES.items() if c.procs)
ONE_WORD_RULES = tuple(n for n, c in CASES.items() if c.cls.rules and not c.procs)

# (n_ops, processes, busy); every third history invalid
MIX = ((8, 3, 0.8), (8, 4, 0.6), (40, 4, 0.5), (40, 6, 0.5), (200, 8, 0.4), (200, 12, 0.3), (600, 16, 0.3), (600, 10, 0.4), (8, 3, 0.7), (40, 5, 0.6),
       (200, 8, 0.5), (600, 16, 0.35))
# crashed cases: (n_ops, processes, busy, info) -- 0 .. 8 crashed calls a history
CRASHED_MIX = ((8, 3, 0.8, 0.1), (8, 4, 0.6, 0.1), (40, 4, 0.5, 0.1), (40, 6, 0.5, 0.08), (200, 8, 0.4, 0.03), (200, 12, 0.3, 0.03), (40, 5, 0.6, 0.1),
               (200, 8, 0.3, 0.04), (8, 3, 0.7, 0.1), (40, 4, 0.4, 0.1), (200, 10, 0.3, 0.03), (200, 8, 0.5, 0.03))
WIDE_MIX = tuple((400, 70, 0.08) for _ in range(8))          # two mask words: 70 processes, 5.6 calls in flight
# case -> first seed (default: a hash of the name).  Pinned where the default left fewer than a third of the histories invalid (a planted read that a
# concurrent write explains): tests/test_state_domain_oracle.py asserts the third, and that the oracle decides every history, for every case
SEEDS = {"dom7-init": 1000, "dom8-init": 1000}


def om(case):
    """the oracle's model"""
    return {"kind": case.kind, "init": case.init}


def gm(case):
    """the library's"""
    return core.make_model(N.MODEL_CAS_REGISTER if case.kind == 1 else N.MODEL_REGISTER, case.init)


def values_of(h):
    f, a, b = np.asarray(h.f), np.asarray(h.a, np.int64), np.asarray(h.b, np.int64)
    v = np.concatenate([a, b[f == N.F_CAS]])
    return v[v != NIL]


def written_values(h):
    """what the ops can make the register hold: a of a :write, b of a :cas"""
    f, a, b = np.asarray(h.f), np.asarray(h.a, np.int64), np.asarray(h.b, np.int64)
    return np.concatenate([a[f == N.F_WRITE], b[f == N.F_CAS]])


def n_crashed(h):
    return int((np.asarray(h.ret_pos) == CRASHED).sum())


def mask_words(hists):
    w = (max(h.n_process for h in hists) + 63) // 64
    return 4 if w == 3 else w


# ---- event rows: (type, process, f, a, b)
def events(rows):
    t, p, f, a, b = (np.array([r[k] for r in rows], dt) for k, dt in enumerate((np.uint8, np.int32, np.uint8, np.int32, np.int32)))
    return columns.EventColumns(t, p, f, a, b)


def rows_of(ev):
    return [(int(ev.type[i]), int(ev.process[i]), int(ev.f[i]), int(ev.a[i]), int(ev.b[i])) for i in range(len(ev))]


def call(p, f, a=NIL, b=0, res=None, typ=N.OK):
    """one call alone in time: its invocation and its completion (a read completes with what it read)"""
    return [(N.INVOKE, p, f, NIL if f == N.F_READ else a, b), (typ, p, f, a if res is None else res, b)]


def relabel(rows, fn):
    """every value v of every row as fn(row, v) (nil stays nil)"""
    out = []
    for r in rows:
        t, p, f, a, b = r
        a2 = a if a == NIL else fn(r, a)
        b2 = fn(r, b) if (f == N.F_CAS and b != NIL) else b
        out.append((t, p, f, a2, b2))
    return out


def with_crashed(rows, at, p, f, a, b=0):
    """a crashed call of a process of its own, invoked at row `at`"""
    at = min(at, len(rows))
    return rows[:at] + [(N.INVOKE, p, f, a, b)] + rows[at:] + [(N.INFO, p, f, a, b)]


def from_synth(n, p, busy, seed, n_values, info=0.0, corrupt=0.0, plain=False, planted=None):
    """the C generator's rows; its planted bad read (n_values + 7) renamed `planted`"""
    kw = dict(read=0.5, write=0.5) if plain else {}
    rows = rows_of(synth.register_events(n_ops=n, n_procs=p, seed=seed, busy=busy, info=info, corrupt=corrupt, n_values=n_values, **kw))
    if corrupt:
        rows = relabel(rows, lambda r, v: planted if v == n_values + 7 else v)
    return rows


def simulate(n_ops, n_procs, seed, init, values, busy, info=0.0, plain=False, stale=False):
    """A register that starts at `init` (in the manner of tests/helpers.multi_register_history): every call takes effect at a random instant
    inside its interval; a :cas that finds another value :fail s; a crashed call takes effect or not.  values: what :write / :cas may put there.
    stale: one completed read two thirds in is given another value of the domain (values and the init)."""
    rng = random.Random(seed)
    state = init
    heap, seq, rows, cur = [], 0, [], {}
    think = (1.0 - busy) / busy
    pid = list(range(n_procs))
    next_pid, issued = n_procs, 0
    domain = list(values) + ([init] if init != NIL and init not in values else [])
    for w in range(n_procs):
        heapq.heappush(heap, (rng.expovariate(1.0 / (think + 0.05)), seq, w, "inv")); seq += 1
    while heap:
        t, _, w, what = heapq.heappop(heap)
        if what == "inv":
            if issued >= n_ops:
                continue
            issued += 1
            r = rng.random()
            f = (N.F_READ if r < 0.5 else N.F_WRITE) if plain else (N.F_READ if r < 1 / 3 else N.F_WRITE if r < 2 / 3 else N.F_CAS)
            if f == N.F_WRITE and not values:
                f = N.F_READ
            a, b = NIL, 0
            if f == N.F_WRITE:
                a = rng.choice(values)
            elif f == N.F_CAS:
                a = state if (state != NIL and rng.random() < 0.6) else rng.choice(domain)
                b = rng.choice(values) if values else init
            crashed = rng.random() < info
            cur[w] = {"f": f, "a": a, "b": b, "crashed": crashed, "effect": (rng.random() < 0.5) if crashed else True, "res": a, "failed": False}
            rows.append((N.INVOKE, pid[w], f, a, b))
            L = 0.02 + rng.expovariate(1.0)
            heapq.heappush(heap, (t + rng.random() * L, seq, w, "eff")); seq += 1
            heapq.heappush(heap, (t + L, seq, w, "ret")); seq += 1
        elif what == "eff":
            c = cur[w]
            if c["effect"]:
                if c["f"] == N.F_READ:
                    c["res"] = state
                elif c["f"] == N.F_WRITE:
                    state = c["a"]
                elif state == c["a"]:
                    state = c["b"]
                else:
                    c["failed"] = True
        else:
            c = cur[w]
            if c["crashed"]:
                rows.append((N.INFO, pid[w], c["f"], c["a"], c["b"]))
                pid[w] = next_pid
                next_pid += 1
            else:
                rows.append((N.FAIL if c["failed"] else N.OK, pid[w], c["f"], c["res"], c["b"]))
            heapq.heappush(heap, (t + rng.expovariate(1.0 / think) + 1e-9, seq, w, "inv")); seq += 1
    if stale:
        reads = [i for i, r in enumerate(rows) if r[0] == N.OK and r[2] == N.F_READ and r[3] != NIL]
        by_crashed = {r[3] for r in rows if r[0] == N.INFO and r[2] == N.F_WRITE} | {r[4] for r in rows if r[0] == N.INFO and r[2] == N.F_CAS}
        other = lambda v: [x for x in domain if x != v and x not in by_crashed]          # (a crashed call could explain what it writes)
        reads = [i for i in reads if other(rows[i][3])]
        if reads:
            i = reads[len(reads) * 2 // 3]
            t, p, f, a, b = rows[i]
            rows[i] = (t, p, f, rng.choice(other(a)), b)
        else:          # a domain of one value: a read of it before anything else happened (only a register that starts at nil can be wrong about it)
            rows = call(n_procs + 1000, N.F_READ, res=domain[0]) + rows
    return rows


def hand_shapes(init, x, y, kind=1):
    """The four hand shapes of a by-init case (x: a value the ops may write, None where there is none; y: another in-domain value, None
    where there is none).  All of at most 8 ops: brute force checks them."""
    R, W, CAS = N.F_READ, N.F_WRITE, N.F_CAS
    wx = x if x is not None else init
    first = call(0, CAS, init, wx) if kind == 1 else call(0, R, res=init)
    # 1: the init is taken (a :cas [init x] that succeeds; a plain register: read) before any write completes, then overwritten
    h1 = first + call(1, R, res=wx) + (call(0, W, x) + call(1, R, res=x) if x is not None else [])
    # 2: a read of the init open across the first write
    if x is not None:
        h2 = [(N.INVOKE, 0, R, NIL, 0), (N.INVOKE, 1, W, x, 0), (N.OK, 1, W, x, 0), (N.OK, 0, R, init, 0)] + call(1, R, res=x) + call(2, R, res=NIL)
    else:
        other = call(1, CAS, init, wx) if kind == 1 else call(1, R, res=init)          # (nothing to write: the read is open across a :cas [init init])
        h2 = [(N.INVOKE, 0, R, NIL, 0)] + other + [(N.OK, 0, R, init, 0)] + call(2, R, res=init)
    # 3: reads of the init and of nil alone, some concurrent: valid with nothing to search
    h3 = [(N.INVOKE, 0, R, NIL, 0), (N.INVOKE, 1, R, NIL, 0), (N.OK, 1, R, init, 0), (N.INVOKE, 2, R, NIL, 0), (N.OK, 0, R, NIL, 0), (N.OK, 2, R, init, 0)] + call(1, R, res=init)
    # 4: a read of another in-domain value before any write -- the history's only flaw
    h4 = (call(0, R, res=y) + call(1, W, y) + call(0, R, res=y)) if y is not None else None
    return [h1, h2, h3] + ([h4] if h4 is not None else [])


def _seed0(name):
    return SEEDS.get(name, 1000 * (sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000))


def _finish(case, rows):
    if case.lo:
        rows = relabel(rows, lambda r, v: v + case.lo)
    return columns.pair_events(events(rows))


@functools.lru_cache(maxsize=None)
def histories(name):
    """the case's histories, as OpColumns"""
    case = CASES[name]
    s0 = _seed0(name)
    mix = WIDE_MIX if case.procs else CRASHED_MIX if case.info else MIX
    plain = case.kind == 0
    out = []
    if case.how == "values":
        span = case.vmax - case.lo + 1                      # the ops hold lo .. vmax: generated as 0 .. span - 1, shifted by lo
        for i, m in enumerate(mix):
            n, p, busy = m[:3]
            info = m[3] if case.info else 0.0
            bad = i % 3 == 0 or i == 10
            if span == 1:                                  # one value: an invalid history reads it before anything was written
                rows = simulate(n, p, s0 + i, NIL, [0], busy, info, plain, stale=bad)
            else:
                rows = from_synth(n, p, busy, s0 + i, span - 1 if bad else span, info, 0.5 if bad else 0.0, plain, planted=span - 1)
            if case.info and case.vmax >= 30 and n >= 40:   # crashed calls that hold the domain's last values: bit 31 of a reach row, the last count classes
                top = case.vmax - case.lo - (1 if bad else 0)          # (an invalid history's planted read holds the last value: nobody may write it)
                rows = with_crashed(rows, len(rows) // 3, 5000, N.F_WRITE, top)
                if not plain:
                    rows = with_crashed(rows, len(rows) // 2, 5001, N.F_CAS, top, (7 * i) % top)
            out.append(_finish(case, rows))
        return tuple(out)
    init = case.init
    top = case.vmax - 2 if init >= 0 else case.vmax          # the ops write 0 .. top (init 31: 0 .. 29; init -1: 0 .. 3)
    values = list(range(0, top + 1))
    x = values[len(values) // 2] if values else None
    y = x if x is not None else None
    hands = hand_shapes(init, x, y, case.kind)
    rest = [m for m in mix]
    if case.procs:
        plan = [("relabel", rest[0], False), ("relabel", rest[1], True), ("sim", rest[2], True), ("sim", rest[3], False)]
    else:
        pick = (2, 4, 6, 1, 3, 5, 7, 10)
        kinds = ("relabel", "relabel", "relabel", "relabel", "sim", "sim", "sim", "sim")
        bads = (False, True, False, False, True, False, True, True)
        plan = [(k, rest[j], bd) for k, j, bd in zip(kinds, pick, bads)]
        if len(hands) < 4:                                   # (no other in-domain value: one more simulated history instead)
            plan.append(("sim", rest[9], False))
    for h in hands:
        out.append(_finish(case, h))
    for i, (k, m, bad) in enumerate(plan):
        n, p, busy = m[:3]
        info = m[3] if case.info else 0.0
        if k == "relabel" and values:
            rows = from_synth(n, p, busy, s0 + i, len(values), info, 0.5 if bad else 0.0, plain, planted=init)
            rows = [(t, pr, f, init if (t == N.OK and f == N.F_READ and a == NIL) else a, b) for (t, pr, f, a, b) in rows]
        else:
            rows = simulate(n, p, s0 + i, init, values, busy, info, plain, stale=bad and len(values) > 0)
        if case.info and case.vmax >= 30 and n >= 40 and not plain:
            rows = with_crashed(rows, len(rows) // 3, 5000, N.F_CAS, init, (7 * i) % (top + 1))
        out.append(_finish(case, rows))
    return tuple(out)


# ---- references, computed once
@functools.lru_cache(maxsize=None)
def _window(name, under_nil=False):
    from oracle import wgl
    case = CASES[name]
    model = {"kind": case.kind, "init": NIL} if under_nil else om(case)
    return tuple(wgl.check(h.as_dict(), model, "window", max_steps=3_000_000) for h in histories(name))


def window_refs(name):
    """oracle.check(..., "window") of every history under the case's model (the budget is tests/test_gpu_parity.py's)"""
    return _window(name)


def window_refs_under_nil(name):
    return _window(name, True)


# ---- hand known-answer histories for the knossos surface: (name, model, Jepsen history, valid?, index of the failing completion, the message
# a final path ends in).  Small enough for oracle/brute.py.
def kats():
    I, K = kop.invoke, kop.ok
    out = []
    out.append(("cas-0-taken-by-a-cas", M.cas_register(0), [I(0, "cas", [0, 1]), K(0, "cas", [0, 1]), I(1, "read", None), K(1, "read", 1)], True, None, None))
    out.append(("cas-3-read-across-the-first-write", M.cas_register(3),
                [I(0, "read", None), I(1, "write", 1), K(1, "write", 1), K(0, "read", 3), I(1, "read", None), K(1, "read", 1)], True, None, None))
    out.append(("cas-3-reads-1-before-any-write", M.cas_register(3), [I(0, "read", None), K(0, "read", 1), I(1, "write", 1), K(1, "write", 1)], False, 1,
                "can't read 1 from register 3"))
    out.append(("cas-0-stale-init-after-a-cas", M.cas_register(0),
                [I(0, "cas", [0, 2]), K(0, "cas", [0, 2]), I(1, "read", None), K(1, "read", 2), I(2, "read", None), K(2, "read", 0)], False, 5, "can't read 0 from register 2"))
    out.append(("register-5-reads-alone", M.register(5), [I(0, "read", None), I(1, "read", None), K(1, "read", 5), K(0, "read", None), I(2, "read", None), K(2, "read", 5)],
                True, None, None))
    out.append(("register-5-stale-init-after-a-write", M.register(5), [I(0, "write", 2), K(0, "write", 2), I(1, "read", None), K(1, "read", 5)], False, 3,
                "can't read 5 from register 2"))
    out.append(("cas-30-the-last-table-value", M.cas_register(30),
                [I(0, "cas", [30, 7]), I(1, "read", None), K(1, "read", 30), K(0, "cas", [30, 7]), I(1, "read", None), K(1, "read", 30)], False, 5,
                "can't read 30 from register 7"))
    # a string-valued init among integer values: the values are interned together (knossos/_analysis.py _Interner), the init is one of them
    out.append(("cas-string-init-among-integers", M.cas_register("a"),
                [I(0, "read", None), K(0, "read", "a"), I(0, "cas", ["a", 1]), K(0, "cas", ["a", 1]), I(1, "read", None), K(1, "read", 1), I(2, "read", None), K(2, "read", "a")],
                False, 7, "can't read a from register 1"))
    return out


# ---- multi-register: 4 bits a key, the init the packed map (knossos/_analysis.py _multi_register_direct)
MR_KEYS = tuple("k%d" % i for i in range(8))
MR_VALUES = tuple(range(100, 114))                 # 14 distinct values: codes 0 .. 13, held as code + 1 in a key's 4 bits
MR_INIT = {"k7": 113, "k0": 100, "k3": 107}        # key 7 at the 14th value: bits 28 .. 31 of the state = 0xE


def multi_register_history(n_ops, n_procs, seed, init=None, keys=MR_KEYS, values=MR_VALUES, busy=0.3, info=0.0, stale=False, read_first=True):
    """As tests/helpers.multi_register_history, from a NON-EMPTY initial map: the store starts as `init`; read_first: the first txn reads
    every key of the initial map before any write is invoked; stale: one completed read two thirds in is given another value of the domain."""
    rng = random.Random(seed)
    state = dict(init or {})
    heap, seq, hist, cur = [], 0, [], {}
    if read_first and init:
        mops = [["r", k, None] for k in init]
        hist.append({"type": "invoke", "f": "txn", "value": [list(m) for m in mops], "process": n_procs})
        hist.append({"type": "ok", "f": "txn", "value": [["r", k, init[k]] for k in init], "process": n_procs})
    think = (1.0 - busy) / busy
    pid = list(range(n_procs))
    next_pid, issued = n_procs + 1, 0
    for w in range(n_procs):
        heapq.heappush(heap, (rng.expovariate(1.0 / (think + 0.05)), seq, w, "inv")); seq += 1
    while heap:
        t, _, w, what = heapq.heappop(heap)
        if what == "inv":
            if issued >= n_ops:
                continue
            issued += 1
            mops = []
            for _ in range(rng.randint(1, 3)):
                k = rng.choice(keys)
                mops.append(["r", k, None] if rng.random() < 0.5 else ["w", k, rng.choice(values)])
            crashed = rng.random() < info
            cur[w] = {"mops": mops, "crashed": crashed, "effect": (rng.random() < 0.5) if crashed else True, "res": None}
            hist.append({"type": "invoke", "f": "txn", "value": [list(m) for m in mops], "process": pid[w]})
            L = 0.02 + rng.expovariate(1.0)
            heapq.heappush(heap, (t + rng.random() * L, seq, w, "eff")); seq += 1
            heapq.heappush(heap, (t + L, seq, w, "ret")); seq += 1
        elif what == "eff":
            c = cur[w]
            if c["effect"]:
                res = []
                for f, k, v in c["mops"]:
                    if f == "r":
                        res.append(["r", k, state.get(k)])
                    else:
                        state[k] = v
                        res.append(["w", k, v])
                c["res"] = res
        else:
            c = cur[w]
            if c["crashed"]:
                hist.append({"type": "info", "f": "txn", "value": [list(m) for m in c["mops"]], "process": pid[w]})
                pid[w] = next_pid
                next_pid += 1
            else:
                hist.append({"type": "ok", "f": "txn", "value": c["res"], "process": pid[w]})
            heapq.heappush(heap, (t + rng.expovariate(1.0 / think) + 1e-9, seq, w, "inv")); seq += 1
    if stale:
        oks = [o for o in hist if o["type"] == "ok" and any(m[0] == "r" and m[2] is not None for m in o["value"])]
        o = oks[len(oks) * 2 // 3]
        m = next(m for m in o["value"] if m[0] == "r" and m[2] is not None)
        m[2] = rng.choice([v for v in values if v != m[2]])
    return hist


def pin_codes(keys, values, process=9000):
    """A first txn that :fail s -- completing the history drops it, it has no effect -- and writes `values` in order to `keys` in turn: the
    encoder numbers keys and values by first appearance (knossos/_analysis.py), so key j gets index j and value j code j, whatever follows."""
    mops = [["w", keys[j % len(keys)], values[j % len(values)]] for j in range(max(len(keys), len(values)))]
    return [{"type": "invoke", "f": "txn", "value": [list(m) for m in mops], "process": process},
            {"type": "fail", "f": "txn", "value": [list(m) for m in mops], "process": process}]


def encode_multi_register(init_map, hist):
    """Two encodings of one history under one initial map -> ((Encoded, library model, oracle model), ...):
    "direct": knossos/_analysis.py's own, Encoded(M.multi_register(map), hist) -- the map's keys and values are numbered FIRST (key 7 of the
              state word holds an initial value only when the map has eight keys, and then a code of at most 7);
    "hand":   the history encoded under the empty map and the init packed here from the same numbering ((code + 1) << 4 * key) -- with
              pin_codes() in front, the map's k7 is key 7 and its value the 14th: bits 28 .. 31 of the init are 0xE."""
    from jepsen_tigerbeetle_amd.knossos import _analysis
    direct = _analysis.Encoded(M.multi_register(dict(init_map)), hist)
    hand = _analysis.Encoded(M.multi_register({}), hist)
    out = []
    for name, enc in (("direct", direct), ("hand", hand)):
        assert enc.native_model[0].kind == N.MODEL_MULTI_REGISTER, name
        init = 0
        for k, v in init_map.items():
            init |= (enc.intern.enc(v) + 1) << (4 * enc.mr_keys[k])
        if init >= 2 ** 31:
            init -= 2 ** 32                                  # (tbc_model.init is an int32: bit 31 of the state word is its sign)
        native = enc.native_model if name == "direct" else core.make_model(N.MODEL_MULTI_REGISTER, init, n_keys=max(1, len(enc.mr_keys)))
        out.append((name, enc, native, {"kind": 4, "init": init, "pool": enc.ops.pool}))
    return out


@functools.lru_cache(maxsize=None)
def multi_register_cases():
    """(name, initial map, Jepsen history): 8 keys, 14 distinct values, 200 .. 400 ops, 8 processes, from a non-empty initial map that holds
    key 7 at the 14th value; every history begins by reading the whole initial map before any write is invoked; half have a planted stale read"""
    out = []
    for i, (n, stale, info) in enumerate(((200, False, 0.0), (300, True, 0.0), (400, False, 0.0), (250, True, 0.0), (200, False, 0.02), (300, True, 0.02))):
        h = pin_codes(MR_KEYS, MR_VALUES[:13]) + multi_register_history(n, 8, 7100 + i, MR_INIT, busy=0.3, info=info, stale=stale)
        out.append(("map-%d%s%s" % (n, "-stale" if stale else "", "-crashed" if info else ""), MR_INIT, h))
    return tuple(out)


def multi_register_fallbacks():
    """(name, initial map, Jepsen history): what the direct model does not hold goes to the memo table -- 15 distinct values; 9 keys.  Small
    enough (at most 8 ops) for brute force over the memo table; seeds with and without a stale read."""
    v15 = tuple(range(100, 115))
    k9 = tuple("k%d" % i for i in range(9))
    out = []
    for s in range(4):
        a = pin_codes(MR_KEYS, v15) + multi_register_history(7, 3, 7300 + s, {"k7": 114}, keys=("k0", "k1", "k7"), values=(100, 101, 114), busy=0.6, stale=s % 2 == 1)
        b = pin_codes(k9, MR_VALUES[:3]) + multi_register_history(7, 3, 7310 + s, {"k8": 101}, keys=("k0", "k1", "k8"), values=MR_VALUES[:3], busy=0.6, stale=s % 2 == 1)
        out += [("15-values-%d" % s, {"k7": 114}, a), ("9-keys-%d" % s, {"k8": 101}, b)]
    return tuple(out)



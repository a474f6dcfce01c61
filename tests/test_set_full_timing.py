"""set-full's scan (csrc/set_full.hip) under the TIMING of reads: slow readers and uneven prefixes.

tests/test_set_full.py and tests/test_set_full_keys.py are broad in shape and narrow in time: a read of theirs completes a handful of
reads after it was invoked.  The reference's nemesis pauses and partitions nodes, so a real set-full history holds reads that take
seconds while hundreds of others come and go.  Only such reads reach
  * the `known` walk of setfull_resolve_kernel past its first 64 rows and past a chunk (the RowsAhead hand-over),
  * chunks whose prefixes P[r] lie far apart (setfull_any_kernel's general path with almost every row masked; a summary that says
    "present here" because of one row),
  * rows and elements that never count, and elements whose only set bits lie above the row's prefix.
`_timed_key` builds keys in the encoder's compact form with the duration of every read chosen by a profile.  CPU tier: the numpy
partner (`_dense_states`) is pinned against oracle/set_full.py on histories with slow reads, and every (shape, profile) is shown, from
numpy alone, to contain what it is for.  GPU tier: KeyedScan == Scan(rows=True) == the dense entry == numpy, bit for bit, twice."""
import functools
import random

import numpy as np
import pytest

from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import set_full as sf
from oracle import set_full as osf
from test_set_full_keys import _Arr, _assert_keyed_equals_single, _dense_states

NONE = N.NO_OP
FIELDS = ("known", "last_present", "last_absent")
PROFILES = ("slow", "sees_everything_first", "reads_before_adds", "phantoms_only", "edges")
# E: 33 / 129 = one bit into the second / fifth word; 4,100 = 129 words, pitch 132, 33 resolve workgroups (no multiple of 8); 33,000 >
# 32,768 = two column blocks.  R: 130 = 2 chunks of 65; 2,049 = 32 chunks of 65 (the last one short; an 8-row unroll remainder of 1);
# 5,000 = 64 chunks of 79 (remainder 7, a last 64-row step of 15).  (33,000 x 2,049 is left out: nothing the others lack.)
SHAPES = [(E, R) for E in (33, 129, 4100, 33000) for R in (130, 2049, 5000) if (E, R) != (33000, 2049)]
# `slow` only: one read that stays open while two whole chunks of other reads come and go (128 chunks of 65 rows at this shape)
LONG_SHAPE, LONG_SPAN = (64, 2048 * 4 + 100), 3 * 65 + 10
# `slow` only: more than 256 chunks (512 of 1,025 rows), where the resolve pass holds no summaries in registers and the `known` walk
# fetches its first rows itself instead of taking them over from the prefetch; one read open over three chunks' worth of reads
MANY_SHAPE, MANY_SPAN = (64, 2048 * 256 + 100), 3 * 1025 + 10
# `edges` only: the one chunking here whose chunks have rows 127 and 128 (256 chunks of 130 rows)
TALL_SHAPE = (96, 256 * 130)


def _chunks(E, R):
    """(chunks, rows per chunk) of a key: what the planner gives it (csrc/set_full_plan.h: sf_chunks and the two lines of sf_make_layout
    that call it), restated so that the generator can aim at chunk boundaries; tests/test_set_full_plan.py holds the planner to it."""
    if not (E and R):
        return 1, max(1, R)
    col_blocks = max(1, ((E + 31) // 32 + 255) // 256)
    chunks = max(1, min(256, 8192 // col_blocks))
    while chunks > 1 and R // chunks < 64:
        chunks >>= 1
    while (R + chunks - 1) // chunks > 2048:
        chunks <<= 1
    return chunks, max(1, (R + chunks - 1) // chunks)


def _edge_positions(rpc):
    """Row positions inside a chunk where `edges` puts a deciding row: the chunk's first and last row, rows 63 / 64 / 65 and 127 / 128
    of it (where the chunk is that long) -- and, because setfull_last_in_chunk steps 64 rows at a time from the chunk's END, the rows
    on either side of those steps."""
    named = {0, rpc - 1, 63, 64, 65, 127, 128}
    steps = {rpc - 64, rpc - 65, rpc - 128, rpc - 129}
    return sorted(p for p in named if 0 <= p < rpc), sorted(p for p in named | steps if 0 <= p < rpc)


def _tail(E):
    """reads_before_adds: how many trailing elements are invoked after the last read completed -- a tenth of them, but at least 40
    (so that whole words of columns never count) where the key has twice that many, else half the key."""
    return min(E, max(E // 10, min(40, E // 2)))


# ---------------------------------------------------------------------------------------------------- the generator
def _timed_key(E, R, seed, profile, span=None):
    """E elements and R reads of a grow-only set on ONE timeline of unique op indices, in the encoder's compact form.  Every op is
    invoked in a slot of its own; a read completes just after the invocation of the read `d` later (d: the profile's choice), an add a
    little after its invocation, or never (add_ok NONE).  A read holds the elements invoked before it completed, less a lag of 0-2 for a
    fast read (a slow one holds everything: the set as of its completion), less 0-3 holes, plus at most one element above that (mostly
    above the row's prefix: a bit that must never count).  Profiles: see the module's docstring and each branch."""
    assert profile in PROFILES
    rng = np.random.default_rng(seed)
    a = _Arr()
    a.E, a.R, a.profile = E, R, profile
    a.wpr = max(1, (E + 31) // 32)
    chunks, rpc = _chunks(E, R)
    n = E + R
    # ---- the slots: which invocations are reads
    kind = np.zeros(n, bool)
    n0 = 0
    if profile == "reads_before_adds" and R:
        # the first third of the reads -- one whole chunk and a few rows where a third is less -- come and go before the first add; the
        # last `tail` elements are invoked after the last read completed
        n0, tail = min(R, max(R // 3, rpc + 3)), _tail(E)
        kind[:n0] = True
        if R > n0:
            kind[n0 + rng.choice(n - n0 - tail, R - n0, replace=False)] = True
    elif R:
        lead = min(R, 3) if profile == "sees_everything_first" else 0          # (reads 1 and 2 complete before any add)
        kind[:lead] = True
        kind[lead + rng.choice(n - lead, R - lead, replace=False)] = True
    t_ai, t_ri = np.nonzero(~kind)[0].astype(np.float64), np.nonzero(kind)[0].astype(np.float64)
    # ---- how long a read lasts, in reads invoked meanwhile
    d = rng.integers(0, 6, R)
    if profile == "slow" and R:
        u = rng.random(R)
        d = np.where(u < 1 / 30, rng.integers(200, 400, R), np.where(u < 1 / 8, rng.integers(64, 200, R), d))
        few = rng.choice(max(1, R - rpc), min(3, max(1, R - rpc)), replace=False)            # a few outlast a whole chunk of later reads
        d[few] = rpc + rng.integers(1, rpc + 1, len(few))
        if span:        # one read stays open over `span` later reads, and the middle element is invoked just before it completes
            a.span_row = int(np.searchsorted(t_ri, t_ai[E // 2])) - (span - 5)
            assert a.span_row >= 0
            d[a.span_row] = span
    slow = d >= 64
    last = np.minimum(np.arange(R) + d, R - 1)
    if n0:
        last[:n0] = np.minimum(last[:n0], n0 - 1)
    t_ro = t_ri[last] + rng.uniform(0.05, 0.95, R)
    if profile == "sees_everything_first" and R:
        t_ro[0], slow[0] = n + 0.5, True                                         # invoked first, completes after every add
    # ---- the adds' acknowledgements: soon, late (so that a read is what makes the element known), or never
    t_ao = t_ai + np.where(rng.random(E) < 0.1, rng.uniform(6.0, 400.0, E), rng.uniform(0.1, 6.0, E))
    never = rng.random(E) < 0.1
    if profile == "reads_before_adds":
        never[E - _tail(E)::3] = True
    if span:
        never[E // 2] = True                          # (never acknowledged: a read is what makes it known)
    # ---- op indices: the rank of every event on the one timeline
    times = np.concatenate([t_ai, t_ri, t_ro, t_ao[~never]])
    rank = np.empty(len(times), np.int64)
    rank[np.argsort(times, kind="stable")] = np.arange(len(times))
    a.add_invoke, a.read_invoke, a.read_ok = (rank[:E].astype(np.uint32), rank[E:E + R].astype(np.uint32), rank[E + R:E + 2 * R].astype(np.uint32))
    a.add_ok = np.full(E, NONE, np.uint32)
    a.add_ok[~never] = rank[E + 2 * R:]
    P = np.searchsorted(a.add_invoke, a.read_ok).astype(np.int64)              # the row's prefix: adds invoked before it completed
    # ---- what a read holds
    top = np.maximum(P - np.where(slow, 0, rng.integers(0, 3, R)), 0)
    k_holes = rng.integers(0, 4, R)
    if profile == "sees_everything_first" and R:
        k_holes[0] = 3
    rows = np.repeat(np.arange(R, dtype=np.int64), k_holes)
    holes = np.floor(rng.random(len(rows)) * top[rows]).astype(np.int64)
    keep = top[rows] > 0
    rows2 = np.nonzero((rng.integers(0, 2, R) == 1) & (top < E))[0].astype(np.int64)
    above = top[rows2] + np.floor(rng.random(len(rows2)) * (E - top[rows2])).astype(np.int64)
    W = E + 1
    key = np.unique(np.concatenate([rows[keep] * W + holes[keep], rows2 * W + above]))      # one exception = row * W + element

    def force(e, want):
        """column e is what `want` says, row by row, whatever the random exceptions made of it"""
        nonlocal key
        flip = np.nonzero(want != (e < top))[0].astype(np.int64)
        key = np.concatenate([key[key % W != e], flip * W + e])

    if profile == "phantoms_only" and E and R:
        # a band of elements no row that counts for them holds: their only set bits are "above" exceptions of rows that completed before
        # their add was invoked (every sixth of them has no bit at all)
        b0, band = E // 3, min(48, E // 2)
        for i, e in enumerate(range(b0, b0 + band)):
            want = (P <= e) & (rng.random(R) < 0.5)
            if i % 6 == 5:
                want[:] = False
            elif (P <= e).any():
                want[np.nonzero(P <= e)[0][0]] = True
            force(e, want)
    if profile == "edges" and E and R:
        # elements vanish and reappear, and the row that decides last-present (the element is in it and in no later row) or last-absent
        # (it is missing from it and in every later row) is put on the named positions of a full chunk in the later half of the reads
        full_chunks = R // rpc
        used, r_all = set(), np.arange(R)
        for p in _edge_positions(rpc)[1]:
            for present in (True, False):
                r = int(rng.integers(full_chunks // 2, full_chunks)) * rpc + p
                free = [e for e in range(int(P[r])) if e not in used]
                assert free, (E, R, seed, "no element invoked before row %d completed is left" % r)
                e = int(rng.choice(free))
                used.add(e)
                if present:      # there, gone for 15 rows, back for the 5 rows up to r, then gone for good
                    want = (r_all < r - 20) | ((r_all >= r - 5) & (r_all <= r))
                else:            # there, gone for the 10 rows up to r, back for good
                    want = (r_all < r - 10) | (r_all > r)
                force(e, want)
    key = np.sort(key)
    a.top = top.astype(np.uint32) if R else np.zeros(1, np.uint32)
    a.exc = (key % W).astype(np.uint32)
    a.exc_off = np.concatenate([[0], np.cumsum(np.bincount(key // W, minlength=R))]).astype(np.uint64)
    return a


def _rows_of(a, op_index, column):
    """the read (row number) whose read_invoke / read_ok is each given op index"""
    col = getattr(a, column).astype(np.int64)
    order = np.argsort(col)
    at = np.minimum(np.searchsorted(col[order], op_index), max(0, a.R - 1))
    assert a.R and (col[order][at] == op_index).all()
    return order[at]


@functools.lru_cache(maxsize=None)
def _cases(profile):
    """the keys of one profile, shuffled, an E = 0 and an R = 0 key among them, and numpy's three indices for each: built once, shared
    by the CPU and the GPU tests of the profile, never written to"""
    at = PROFILES.index(profile)
    keys = [_timed_key(E, R, 100 * at + i, profile) for i, (E, R) in enumerate(SHAPES)]
    if profile == "slow":
        keys.append(_timed_key(*LONG_SHAPE, 100 * at + 50, profile, span=LONG_SPAN))
        keys.append(_timed_key(*MANY_SHAPE, 100 * at + 52, profile, span=MANY_SPAN))
    if profile == "edges":
        keys.append(_timed_key(*TALL_SHAPE, 100 * at + 51, profile))
    keys += [_timed_key(0, 7, 100 * at + 60, profile), _timed_key(9, 0, 100 * at + 61, profile)]
    random.Random(at).shuffle(keys)
    return keys, [_dense_states(k) for k in keys]


# ---------------------------------------------------------------------------------------------------- CPU tier: the reference
def _slow_history(n_adds, n_reads, seed, style):
    """A grow-only set as op maps, from a small event simulation in which a read may stay open for a long time: every op has an
    invocation, an instant inside its interval at which it takes effect, and a completion.  style "slow": one read in five lasts as
    long as 20-120 other ops and shows the set as of its completion; "reads_before_adds": a third of the reads come and go before the
    first add, and the last tenth of the adds is invoked after the last read completed.  Some adds crash (:info), some are
    acknowledged late, and a read now and then misses an element."""
    rng = random.Random(seed)
    kinds = ["add"] * n_adds + ["read"] * n_reads
    if style == "slow":
        rng.shuffle(kinds)
    else:
        early, late = n_reads // 3, max(1, n_adds // 10)
        mid = ["add"] * (n_adds - late) + ["read"] * (n_reads - early)
        rng.shuffle(mid)
        kinds = ["read"] * early + ["gap"] + mid + ["gap"] + ["add"] * late
    events, t, nxt, late_now = [], 0.0, 9, False
    for i, f in enumerate(kinds):
        if f == "gap":                               # longer than any op of this style lasts: everything open completes here
            t += 10.0
            late_now = i > n_reads // 3
            continue
        t += rng.uniform(0.5, 1.0)
        if f == "add":
            dur, crash = (rng.uniform(5, 60) if rng.random() < 0.15 else rng.uniform(0.1, 3)), rng.random() < (0.3 if late_now else 0.08)
            eff, val = t + rng.random() * dur, nxt
            nxt += 1
        else:
            long_ = style == "slow" and rng.random() < 0.2
            dur, crash, val = (rng.uniform(20, 120) if long_ else rng.uniform(0.1, 3)), False, None
            eff = t + (0.99 if long_ else rng.random()) * dur
        if style != "slow":
            dur = min(dur, 3.0)
            eff = min(eff, t + dur * 0.99)
        events += [(t, 0, i, f, val, crash), (eff, 1, i, f, val, crash), (t + dur, 2, i, f, val, crash)]
    state, hist, proc, result, free, n_proc = set(), [], {}, {}, [], 0
    for _, what, i, f, val, crash in sorted(events):
        if what == 0:
            if not free:
                free.append(n_proc)
                n_proc += 1
            proc[i] = free.pop()
            hist.append({"type": "invoke", "f": f, "value": val, "process": proc[i]})
        elif what == 1:
            if f == "add":
                if not crash or rng.random() < 0.5:
                    state.add(val)
            else:
                result[i] = sorted(x for x in state if rng.random() >= 0.01)
        elif crash:
            hist.append({"type": "info", "f": f, "value": val, "process": proc[i], "error": "timeout"})        # (the process is gone)
        else:
            hist.append({"type": "ok", "f": f, "value": val if f == "add" else result[i], "process": proc[i]})
            free.append(proc[i])
    return [dict(o, index=i) for i, o in enumerate(hist)]


def _history_of_key(a):
    """the op maps that encode to key `a`: every index of its one timeline is one op (element e is the value e + 9)"""
    ev = [(int(i), "invoke", "add", e) for e, i in enumerate(a.add_invoke)] + [(int(i), "ok", "add", e) for e, i in enumerate(a.add_ok) if i != NONE]
    ev += [(int(i), "invoke", "read", r) for r, i in enumerate(a.read_invoke)] + [(int(i), "ok", "read", r) for r, i in enumerate(a.read_ok)]
    hist, free, proc, n_proc = [], [], {}, 0
    for i, (index, typ, f, x) in enumerate(sorted(ev)):
        assert index == i
        if typ == "invoke":
            if not free:
                free.append(n_proc)
                n_proc += 1
            proc[f, x] = free.pop()
            hist.append({"type": "invoke", "f": f, "value": x + 9 if f == "add" else None, "process": proc[f, x], "index": i})
            continue
        free.append(proc[f, x])
        value = x + 9
        if f == "read":
            row = np.arange(a.E) < a.top[x]
            row[a.exc[int(a.exc_off[x]):int(a.exc_off[x + 1])]] ^= True
            value = [int(e) + 9 for e in np.nonzero(row)[0]]
        hist.append({"type": "ok", "f": f, "value": value, "process": proc[f, x], "index": i})
    return hist


def _assert_numpy_equals_oracle(h, what):
    enc = sf.Encoded(h)
    got, want = _dense_states(enc), osf.element_states(h)
    assert enc.elements == [w["element"] for w in want], what
    for f in FIELDS:
        assert [int(x) for x in got[f]] == [w[f] for w in want], (what, f)
    return enc, got


def test_numpy_reference_equals_the_oracle_on_histories_with_slow_reads():
    """`_dense_states` is the device scan's independent partner on every key below, so it has to be right where reads are slow: field
    by field against the fold of oracle/set_full.py, on simulated histories of a few hundred ops ..."""
    for seed in range(6):
        h = _slow_history(150, 250, seed, "slow")
        enc, got = _assert_numpy_equals_oracle(h, ("slow", seed))
        # (the history is what it claims to be: some read stayed open while 20 others were invoked, and some element became known
        # through a read that is not the first, by invocation, to hold it)
        assert (np.searchsorted(enc.read_invoke, enc.read_ok) - np.arange(enc.R) > 20).sum() >= 10, seed
        assert len(_overtaken(enc, got)[0]) >= 5, seed
    for seed in range(6):
        h = _slow_history(200, 200, 10 + seed, "reads_before_adds")
        enc, got = _assert_numpy_equals_oracle(h, ("reads_before_adds", seed))
        assert (np.searchsorted(enc.add_invoke, enc.read_ok) == 0).sum() >= 60, seed
        late = enc.add_invoke > enc.read_ok.max()
        assert late.sum() >= 15 and (got["last_present"][late] == NONE).all() and (got["last_absent"][late] == NONE).all(), seed
        assert (enc.add_ok[late] == NONE).any() and np.array_equal(got["known"][late], enc.add_ok[late]), seed


@pytest.mark.parametrize("profile", PROFILES)
def test_numpy_reference_equals_the_oracle_on_the_generated_keys(profile):
    """... and on the generator's own keys, turned back into op maps: the smallest shapes of every profile, bits above a row's prefix
    (values a read holds before anybody added them) included.  The op maps encode to the key's four index columns again."""
    for E, R in ((33, 130), (129, 130), (129, 2049)):
        a = _timed_key(E, R, 7 + E + R, profile)
        enc, got = _assert_numpy_equals_oracle(_history_of_key(a), (profile, E, R))
        for f in ("add_invoke", "add_ok", "read_invoke", "read_ok"):
            assert np.array_equal(getattr(enc, f), getattr(a, f)), (profile, E, R, f)
        mine = _dense_states(a)
        for f in FIELDS:
            assert np.array_equal(got[f], mine[f]), (profile, E, R, f)


def _overtaken(a, ref):
    """The elements that became known through a read that is NOT the first read, in invocation order, to hold them: -> (elements, row
    of that first read, row of the read that made them known).  The first holder is min read_invoke over the rows that hold the element
    and count for it -- `_dense_states`' own last-present reduction, over the same key with the invocation order mirrored."""
    BIG = 1 << 31
    m = _Arr()
    m.__dict__.update(a.__dict__)
    m.read_invoke = (BIG - a.read_invoke.astype(np.int64)).astype(np.uint32)
    lp = _dense_states(m)["last_present"]
    by_read = (ref["known"] != NONE) & (ref["known"] != a.add_ok) & (lp != NONE)
    el = np.nonzero(by_read)[0]
    if not len(el):
        return el, el, el
    first = _rows_of(a, BIG - lp[el].astype(np.int64), "read_invoke")
    decides = _rows_of(a, ref["known"][el].astype(np.int64), "read_ok")
    assert (decides >= first).all()
    keep = decides != first
    return el[keep], first[keep], decides[keep]


def _real(keys, refs):
    return [(a, ref, _chunks(a.E, a.R)[1], np.searchsorted(a.add_invoke, a.read_ok)) for a, ref in zip(keys, refs) if a.E and a.R]


def _atleast(n, room):
    """A count this file asks of a key (`n`) wherever the key has room for it; a key of fewer elements owes `room`, a share of its own."""
    return min(n, room)


def test_slow_keys_have_reads_overtaken_across_steps_and_chunks():
    """every `slow` key: 50 elements became known through a read other than their first holder; for 10 of them that read lies 64 or
    more rows later, i.e. in a later step of the `known` walk, for 3 in a later chunk.  (Keys of fewer than 100 elements -- 33, and the
    long key's 64 -- cannot be asked for 50: a quarter and a sixteenth of their elements instead.)  The long key: one read stays open
    while three chunks' worth of reads are invoked, and some element's first holder and deciding read have two whole chunks between."""
    keys, refs = _cases("slow")
    for a, ref, rpc, P in _real(keys, refs):
        el, first, decides = _overtaken(a, ref)
        what = (a.E, a.R, len(el), int((decides - first >= 64).sum()), int((decides // rpc > first // rpc).sum()))
        small = a.E < 100
        assert len(el) >= (a.E // 4 if small else 50), what
        assert (decides - first >= 64).sum() >= (a.E // 16 if small else 10), what
        assert (decides // rpc > first // rpc).sum() >= 3, what
        if (a.E, a.R) in (LONG_SHAPE, MANY_SHAPE):
            r = a.span_row
            open_over = np.searchsorted(a.read_invoke, a.read_ok[r]) - r            # reads invoked while read r was open
            assert rpc == (65 if (a.E, a.R) == LONG_SHAPE else 1025) and open_over >= 3 * rpc, (what, open_over)
            assert (decides // rpc - first // rpc >= 3).any(), what


def test_one_slow_first_read_spreads_the_prefixes_of_chunk_0():
    keys, refs = _cases("sees_everything_first")
    for a, ref, rpc, P in _real(keys, refs):
        assert P[:rpc].max() == P[0] == a.E and P[1:rpc].min() <= 32, (a.E, a.R)
        assert a.read_invoke[0] < a.add_invoke[0] and a.read_ok[0] > a.add_invoke[-1], (a.E, a.R)
        assert a.top[0] == a.E and 1 <= a.exc_off[1] <= 3, (a.E, a.R)                  # row 0 holds everything but a few holes


def test_early_reads_and_late_adds_never_count():
    keys, refs = _cases("reads_before_adds")
    for a, ref, rpc, P in _real(keys, refs):
        assert (P[:rpc] == 0).all() and (P[:a.R // 3] == 0).all(), (a.E, a.R)         # a whole chunk, and a third of the reads
        tail = _tail(a.E)
        late = np.arange(a.E) >= a.E - tail
        assert tail >= _atleast(32, a.E // 3) and (a.add_invoke[late] > a.read_ok.max()).all(), (a.E, a.R)
        assert (ref["last_present"][late] == NONE).all() and (ref["last_absent"][late] == NONE).all(), (a.E, a.R)
        assert np.array_equal(ref["known"][late], a.add_ok[late]) and (a.add_ok[late] == NONE).sum() >= tail // 3, (a.E, a.R)
        assert (ref["last_absent"][~late] != NONE).any()


def test_phantom_band_is_present_somewhere_and_never_counts():
    keys, refs = _cases("phantoms_only")
    for a, ref, rpc, P in _real(keys, refs):
        rows = np.repeat(np.arange(a.R), np.diff(a.exc_off.astype(np.int64)))
        ever = np.zeros(a.E, bool)
        ever[a.exc[a.exc >= a.top[rows]]] = True                                       # an "above" exception is a set bit
        band = min(48, a.E // 2)
        ghosts = ever & (ref["last_present"] == NONE) & (ref["last_absent"] != NONE)
        assert ghosts.sum() >= _atleast(40, band - band // 6), (a.E, a.R, int(ghosts.sum()))


def test_edges_put_the_deciding_rows_on_the_named_positions():
    keys, refs = _cases("edges")
    seen_tall = False
    for a, ref, rpc, P in _real(keys, refs):
        named = _edge_positions(rpc)[0]
        for f in ("last_present", "last_absent"):
            has = ref[f] != NONE
            at = set((_rows_of(a, ref[f][has].astype(np.int64), "read_invoke") % rpc).tolist())
            assert set(_edge_positions(rpc)[1]) <= at, (a.E, a.R, f, sorted(set(_edge_positions(rpc)[1]) - at))
        seen_tall |= {127, 128} <= set(named)
        assert {0, rpc - 1, 63, 64} <= set(named)
    assert seen_tall


# ---------------------------------------------------------------------------------------------------- GPU tier
def _dense_entry(a, wpr):
    """key `a` for tbc_setfull_create: the matrix built on the host, rows of `wpr` words"""
    d = _Arr()
    d.__dict__.update(a.__dict__)
    d.wpr = wpr
    bits = np.zeros((max(a.R, 1), wpr * 32), bool)
    if a.R and a.E:
        bits[:, :a.E] = np.arange(a.E, dtype=np.uint32)[None, :] < a.top[:a.R, None]
        rows = np.repeat(np.arange(a.R), np.diff(a.exc_off.astype(np.int64)))
        bits[rows, a.exc] ^= True
    d.present = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint32))
    return d


def _same(got, want, what):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, "element %d: %d, numpy %d (%d differ)" % (bad[0], got[f][bad[0]], want[f][bad[0]], len(bad)))


@pytest.mark.gpu
@pytest.mark.parametrize("profile", PROFILES)
def test_scan_equals_numpy_whatever_the_reads_timing(native, profile):
    """All keys of a profile in one object: KeyedScan == single-key Scan(rows=True) == tbc_setfull_create on the matrix built on the
    host (rows of a multiple of four words, and of one word more) == numpy, bit for bit; every object run twice."""
    keys, refs = _cases(profile)
    per, _ = _assert_keyed_equals_single(keys, dense_limit=0)
    for a, got, ref in zip(keys, per, refs):
        _same(got, ref, (profile, a.E, a.R, "keyed"))
    with sf.KeyedScan(keys) as ks:
        one, two = ks.run()[0], ks.run()[0]
    for a, x, y, ref in zip(keys, one, two, refs):
        _same(x, ref, (profile, a.E, a.R, "keyed, first run"))
        _same(y, ref, (profile, a.E, a.R, "keyed, second run"))
    for a, ref in zip(keys, refs):
        w4 = (a.wpr + 3) // 4 * 4
        wide = _dense_entry(a, w4 + 1)
        for wpr in (w4, w4 + 1):
            d = wide
            if wpr == w4:
                d = _Arr()
                d.__dict__.update(wide.__dict__)
                d.wpr, d.present = w4, np.ascontiguousarray(wide.present[:, :w4])
            with sf.Scan(d, rows=False) as s:
                one, two = s.run(), s.run()
            _same(one, ref, (profile, a.E, a.R, "dense entry, %d words a row" % wpr))
            _same(two, ref, (profile, a.E, a.R, "dense entry, %d words a row, second run" % wpr))
        with sf.Scan(a, rows=True) as s:
            one, two = s.run(), s.run()
        _same(one, ref, (profile, a.E, a.R, "compact rows"))
        _same(two, ref, (profile, a.E, a.R, "compact rows, second run"))

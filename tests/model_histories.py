"""Seeded histories of the two device models that had none: TBC_MODEL_MUTEX (a simulated lock server) and TBC_MODEL_TABLE (the memo
table of knossos.model.memo: the bank that forbids overdrafts, a set whose adds repeat an element), the shapes the device tests run
them at, and references() -- every case encoded, its shape asserted (mask words, calls in flight, crashed calls, table size, the share
of invocations that survive) and answered once by the sequential oracle.  A plain module like perf_histories.py / ledger_histories.py."""
import heapq
import random

import numpy as np

from helpers import Refused, _simulate, op_tuples
from jepsen_tigerbeetle_amd import _native as N, columns, core
from jepsen_tigerbeetle_amd.knossos import _analysis, memo as memo_ns, model as M

CRASHED = 0xFFFFFFFF
MAX_STEPS, MAX_PROBES = 5_000_000, 20_000_000          # what every reference here must finish within: no case is left out of a comparison
MUTEX, MUTEX_HELD = {"kind": 2, "init": 0}, {"kind": 2, "init": 1}


def mutex_history(n_ops, n_procs, seed, busy, info=0.0, corrupt=None, held_at_start=False, corrupt_at=2 / 3):
    """A lock server.  A worker that holds the lock invokes :release, any other :acquire.  An acquire reaches the server somewhere in
    the first half of its interval and waits there until the lock is free -- several are open at once; it takes effect at the instant
    it is granted, and one that is still waiting when its interval ends completes :fail.  A crashed call (:info) takes effect with
    probability 1/2; its worker goes on under a new process number and, knowing the simulation's truth, releases what it holds.
    The lock is held briefly next to the time a worker spends away from it (it is wanted about half of the time, however many workers
    there are), so that most acquires are granted: failed calls disappear when the history is completed.
    corrupt = "double-acquire" plants a second :ok :acquire by a new process right after a late :ok :acquire (the lock is held there),
    "lost-release" turns a late :ok :release into :fail ("late": corrupt_at of the way through; an open crashed :release explains either, so
    histories with crashed calls plant theirs early).  held_at_start: worker 0 holds the lock and begins with a release (init = 1)."""
    rng = random.Random(seed)
    think = (1.0 - busy) / busy
    hold = min(1.0, (think + 1.0) / (3.0 * n_procs))          # the scale of everything a holder does: answer, time away, release
    heap, hist = [], []
    seq = [0]
    pid = list(range(n_procs))
    next_pid = n_procs
    holder = 0 if held_at_start else None
    waiters, cur, issued = [], {}, 0

    def push(t, w, kind):
        heapq.heappush(heap, (t, seq[0], w, kind)); seq[0] += 1

    def grant(t, w):
        # the server answers at once; a live client has its :ok shortly after (a crashed one times out as it would have)
        cur[w]["granted"] = True
        if not cur[w]["crashed"]:
            cur[w]["ret_at"] = t + (0.01 + rng.expovariate(1.0)) * 0.5 * hold
            push(cur[w]["ret_at"], w, "ret")
        return w

    for w in range(n_procs):
        push(0.0 if (held_at_start and w == 0) else 1e-6 + rng.expovariate(1.0 / (think + 0.05)), w, "inv")
    while heap:
        t, _, w, kind = heapq.heappop(heap)
        if kind == "inv":
            if issued >= n_ops:
                continue
            issued += 1
            f = "release" if holder == w else "acquire"
            crashed = rng.random() < info
            effect = (rng.random() < 0.5) if crashed else True
            L = (0.02 + rng.expovariate(1.0)) * (hold if f == "release" else 1.0)
            cur[w] = {"f": f, "crashed": crashed, "granted": False, "ret_at": t + L}
            hist.append({"type": "invoke", "f": f, "value": None, "process": pid[w]})
            if effect:
                push(t + rng.random() * L * (1.0 if f == "release" else 0.5), w, "eff" if f == "release" else "arrive")
            push(t + L, w, "ret")
        elif kind == "arrive":
            if holder is None:
                holder = grant(t, w)
            else:
                waiters.append(w)
        elif kind == "eff":
            assert holder == w
            holder = None
            if waiters:
                holder = grant(t, waiters.pop(rng.randrange(len(waiters))))
        else:
            c = cur[w]
            if c["ret_at"] != t:
                continue          # (the time-out of an acquire that was granted before it)
            if w in waiters:
                waiters.remove(w)
            if c["crashed"]:
                hist.append({"type": "info", "f": c["f"], "value": None, "process": pid[w], "error": "timeout"})
                pid[w] = next_pid
                next_pid += 1
            else:
                ok = c["f"] == "release" or c["granted"]
                hist.append({"type": "ok" if ok else "fail", "f": c["f"], "value": None, "process": pid[w]})
            push(t + rng.expovariate(1.0 / think) * (0.5 * hold / max(think, 1e-9) if holder == w else 1.0) + 1e-9, w, "inv")
    if corrupt == "lost-release":
        rel = [o for o in hist if o["type"] == "ok" and o["f"] == "release"]
        if rel:
            rel[min(len(rel) - 1, int(len(rel) * corrupt_at))]["type"] = "fail"
    elif corrupt == "double-acquire":
        acq = [i for i, o in enumerate(hist) if o["type"] == "ok" and o["f"] == "acquire"]
        if acq:
            i = acq[min(len(acq) - 1, int(len(acq) * corrupt_at))]
            hist[i + 1:i + 1] = [{"type": "invoke", "f": "acquire", "value": None, "process": next_pid},
                                 {"type": "ok", "f": "acquire", "value": None, "process": next_pid}]
    elif corrupt:
        raise ValueError(corrupt)
    return hist


MUTEX_CORRUPT = "double-acquire"          # of the two, the one the oracle finds invalid more often (tests/test_models_oracle.py counts both)


def table_history(n_ops, n_procs, seed, busy=0.15, info=0.0, corrupt=False, start=4, corrupt_at=2 / 3):
    """The bank that forbids overdrafts: accounts 1..3 start at `start`, transfers of 1..3 between them, one that would overdraw
    completes :fail; a read returns every balance.  corrupt puts one balance of the read `corrupt_at` of the way through off by one
    (the sum no longer adds up: no interleaving explains it)."""
    accounts = (1, 2, 3)
    bal = {a: start for a in accounts}

    def make_op(rng, _):
        if rng.random() < 0.5:
            d, c = rng.sample(accounts, 2)
            return "transfer", {"debit-acct": d, "credit-acct": c, "amount": rng.randint(1, 3)}
        return "read", None

    def apply_op(f, v):
        if f == "read":
            return dict(bal)
        if bal[v["debit-acct"]] < v["amount"]:
            return Refused
        bal[v["debit-acct"]] -= v["amount"]
        bal[v["credit-acct"]] += v["amount"]
        return v

    hist = _simulate(n_ops, n_procs, seed, busy, info, make_op, apply_op)
    if corrupt:
        reads = [o for o in hist if o["type"] == "ok" and o["f"] == "read"]
        if reads:
            o = reads[min(len(reads) - 1, int(len(reads) * corrupt_at))]
            o["value"] = dict(o["value"])
            o["value"][accounts[0]] += 1
    return hist


def table_model(start=4):
    return M.Bank(tuple((a, start) for a in (1, 2, 3)), False)


def set_table_history(n_ops, n_procs, seed, busy=0.3, info=0.0, corrupt=False, n_elems=5):
    """The other way into the memo table: a set whose adds repeat an element (five elements, so at most 32 states; the first two
    invocations add the same one).  corrupt drops
    an element from a late non-empty read."""
    state = set()

    def make_op(rng, issued):
        if issued <= 2:
            return "add", 0          # the repeat that keeps the history off the direct set model, whatever the seed
        return ("add", rng.randrange(n_elems)) if rng.random() < 0.5 else ("read", None)

    def apply_op(f, v):
        if f == "add":
            state.add(v)
            return v
        return sorted(state)

    hist = _simulate(n_ops, n_procs, seed, busy, info, make_op, apply_op)
    if corrupt:
        reads = [o for o in hist if o["type"] == "ok" and o["f"] == "read" and o["value"]]
        if reads:
            o = reads[len(reads) * 2 // 3]
            o["value"] = o["value"][:-1]
    return hist


# ---- encoding: the library's own encoder, the oracle's model beside it
def encode_mutex(hist, held=False):
    enc = _analysis.Encoded(M.Mutex(held), hist)
    assert enc.native_model[0].kind == N.MODEL_MUTEX and enc.native_model[0].init == (1 if held else 0)
    return enc, (MUTEX_HELD if held else MUTEX)


def encode_table(hist, model=None):
    """-> (Encoded, oracle model): the memo table, never a direct device model (MemoTooLarge is not caught: the shapes here fit)."""
    enc = _analysis.Encoded(model if model is not None else table_model(), hist)
    assert enc.native_model[0].kind == N.MODEL_TABLE
    return enc, {"kind": 3, "init": 0, "table": enc.table_info["table"]}


def encode_set_table(hist):
    assert len(hist) < 400          # (under 200 ops)
    return encode_table(hist, M.set())


# ---- shape helpers
def peak_open(ops):
    """the most calls open at one position of the history (a crashed call stays open to the end)"""
    ret = np.where(np.asarray(ops.ret_pos) == CRASHED, ops.n_events, np.asarray(ops.ret_pos)).astype(np.int64)
    d = np.zeros(ops.n_events + 2, np.int64)
    np.add.at(d, np.asarray(ops.inv_pos, np.int64), 1)
    np.add.at(d, ret, -1)
    return int(np.cumsum(d).max()) if len(ops) else 0


def n_crashed(ops):
    return int((np.asarray(ops.ret_pos) == CRASHED).sum())


def mask_words(ops):
    """1, 2, 4 or 8 (= more than 4: the sequential kernel's alone) by the process slots of the history"""
    return 1 if ops.n_process <= 64 else 2 if ops.n_process <= 128 else 4 if ops.n_process <= 256 else 8


def survived(hist, ops):
    """the share of the invocations that are ops after completion (failed calls disappear)"""
    return len(ops) / max(1, sum(1 for o in hist if o["type"] == "invoke"))


# ---- the medium shapes: every mask width, with and without crashed calls, valid and corrupted.
# (name, model, mask words, generator arguments, crashed calls?, corrupted?).  Sizes and rates are chosen so that the sequential oracle
# ends inside MAX_STEPS on every one of them: an invalid history has to be searched exhaustively and every crashed call that is open
# doubles what there is to search, so corrupted histories with crashed calls are short, and a corrupted table history keeps few calls in flight.
SHAPES = [
    ("mutex-1", "mutex", 1, dict(n_ops=400, n_procs=8, busy=0.5), False, False),
    ("mutex-1-bad", "mutex", 1, dict(n_ops=400, n_procs=8, busy=0.5, corrupt=MUTEX_CORRUPT), False, True),
    ("mutex-1-crashes", "mutex", 1, dict(n_ops=300, n_procs=8, busy=0.5, info=0.03), True, False),
    ("mutex-1-crashes-bad", "mutex", 1, dict(n_ops=300, n_procs=8, busy=0.5, info=0.03, corrupt=MUTEX_CORRUPT, corrupt_at=0.1), True, True),
    ("mutex-sweep-crashes", "mutex", 1, dict(n_ops=500, n_procs=8, busy=0.5, info=0.012), True, False),          # (few enough for the sweep's LDS sets)
    ("mutex-held-1", "mutex-held", 1, dict(n_ops=300, n_procs=8, busy=0.5, info=0.02, held_at_start=True), True, False),
    ("mutex-held-1-bad", "mutex-held", 1, dict(n_ops=300, n_procs=8, busy=0.5, corrupt=MUTEX_CORRUPT, held_at_start=True), False, True),
    ("mutex-2", "mutex", 2, dict(n_ops=1200, n_procs=100, busy=0.3), False, False),
    ("mutex-2-bad", "mutex", 2, dict(n_ops=1200, n_procs=100, busy=0.3, corrupt=MUTEX_CORRUPT), False, True),
    ("mutex-2-crashes", "mutex", 2, dict(n_ops=190, n_procs=40, busy=0.3, info=0.45), True, False),
    ("mutex-2-crashes-bad", "mutex", 2, dict(n_ops=400, n_procs=70, busy=0.1, info=0.04, corrupt=MUTEX_CORRUPT, corrupt_at=0.1), True, True),
    ("mutex-4", "mutex", 4, dict(n_ops=2000, n_procs=200, busy=0.3), False, False),
    ("mutex-4-bad", "mutex", 4, dict(n_ops=2000, n_procs=200, busy=0.3, corrupt=MUTEX_CORRUPT), False, True),
    ("mutex-4-crashes", "mutex", 4, dict(n_ops=600, n_procs=150, busy=0.05, info=0.05), True, False),
    ("mutex-8", "mutex", 8, dict(n_ops=2100, n_procs=280, busy=0.2), False, False),
    ("mutex-8-bad", "mutex", 8, dict(n_ops=2100, n_procs=280, busy=0.2, corrupt=MUTEX_CORRUPT), False, True),
    ("table-1", "table", 1, dict(n_ops=600, n_procs=8, busy=0.15), False, False),
    ("table-1-bad", "table", 1, dict(n_ops=600, n_procs=8, busy=0.15, corrupt=True), False, True),
    ("table-1-crashes", "table", 1, dict(n_ops=600, n_procs=8, busy=0.15, info=0.02), True, False),
    ("table-1-crashes-bad", "table", 1, dict(n_ops=200, n_procs=8, busy=0.15, info=0.02, corrupt=True), True, True),
    ("table-sweep-crashes", "table", 1, dict(n_ops=400, n_procs=8, busy=0.15, info=0.008), True, False),          # (levels of at most 64 configs)
    ("table-1-wide", "table", 1, dict(n_ops=2000, n_procs=64, busy=0.15), False, False),
    ("table-2", "table", 2, dict(n_ops=1500, n_procs=100, busy=0.03, info=0.008), True, False),
    ("table-2-bad", "table", 2, dict(n_ops=1500, n_procs=100, busy=0.03, corrupt=True), False, True),
    ("table-4", "table", 4, dict(n_ops=2000, n_procs=200, busy=0.02, info=0.005), True, False),
    ("table-4-bad", "table", 4, dict(n_ops=2000, n_procs=200, busy=0.02, corrupt=True, corrupt_at=0.2), False, True),
    ("table-8", "table", 8, dict(n_ops=2100, n_procs=270, busy=0.02, info=0.0025), True, False),
    ("table-8-bad", "table", 8, dict(n_ops=2100, n_procs=270, busy=0.02, corrupt=True, corrupt_at=0.1), False, True),
    ("set-table", "set-table", 1, dict(n_ops=180, n_procs=6, busy=0.3, info=0.02), True, False),
    ("set-table-bad", "set-table", 1, dict(n_ops=180, n_procs=6, busy=0.3, corrupt=True), False, True),
]
SEEDS = (0, 1)
# The least calls in flight at the busiest moment, per shape (default 4: there is something to search).  The wide masks are to be used by
# many calls open at once, not by slot numbers alone: the crash-free mutex shapes at 2 / 4 / more mask words keep their workers busy
# (about a fifth of 100, a sixth of 200 / 280 with a call open at the peak), the crashed shapes have their crashed calls open to the end.
MIN_PEAK = {"mutex-2": 16, "mutex-2-bad": 16, "mutex-4": 24, "mutex-4-bad": 24, "mutex-8": 24, "mutex-8-bad": 24,
            "mutex-2-crashes": 60, "mutex-2-crashes-bad": 16, "mutex-4-crashes": 24,
            "table-1-wide": 12, "table-2": 12, "table-4": 12, "table-8": 12}


class Case:
    """One history of a shape: name, model ("mutex" / "mutex-held" / "table" / "set-table"), the Jepsen history, its op columns, the
    library's model (`native`) and the oracle's (`om`) and `ref`, the sequential oracle's answer.  The table cases of one model share
    ONE table (a batch has one tbc_model): `ops` holds the classes of that table, `states` its decoded states."""

    def __init__(self, name, model, hist, ops, native, om, states=None):
        self.name, self.model, self.hist, self.ops, self.native, self.om, self.states = name, model, hist, ops, native, om, states
        self.ref = None
        self.peak, self.crashed = peak_open(ops), n_crashed(ops)

    @property
    def is_mutex(self):
        return self.model.startswith("mutex")

    def d(self):
        return self.ops.as_dict()

    def tuples(self):
        return op_tuples(self.ops)


# ---- one memo table for every history of a model: all the calls the model can meet, not just one history's
_TABLES = {}


def universal_table(model):
    """memo() over EVERY class of the model -- bank: the 18 transfers, a read of each reachable state, a read of nothing, and one read
    that no state allows (where a corrupted read goes); set of five elements: the adds, a read of every subset -- so that histories
    encoded one by one (each with the classes it happens to hold) can be renumbered to one table and share a batch."""
    if model not in _TABLES:
        if model == "table":
            m = table_model()
            ops = [{"f": "transfer", "value": {"debit-acct": d, "credit-acct": c, "amount": a}} for d in (1, 2, 3) for c in (1, 2, 3) if c != d for a in (1, 2, 3)]
            reads = [{"f": "read", "value": dict(st.balances)} for st in memo_ns.memo(m, ops)["states"]]
            never = {"f": "read", "value": {1: 5, 2: 4, 3: 4}}
        else:
            m = M.set()
            ops = [{"f": "add", "value": e} for e in range(5)]
            reads = [{"f": "read", "value": sorted(st.s)} for st in memo_ns.memo(m, ops)["states"]]
            never = {"f": "read", "value": [99]}
        info = memo_ns.memo(m, ops + reads + [{"f": "read", "value": None}, never])
        info["never"] = info["classes"][memo_ns.op_class_key(never)]
        assert (info["table"][:, info["never"]] == 0xFFFF).all()
        _TABLES[model] = info
    return _TABLES[model]


def recode(enc, info):
    """enc's op columns with its table's classes renumbered to info's.  A class info does not know must be one no state allows."""
    own = enc.table_info
    remap = np.zeros(max(1, len(own["class_ops"])), np.int32)
    for k, op in enumerate(own["class_ops"]):
        j = info["classes"].get(memo_ns.op_class_key(op))
        if j is None:
            assert (own["table"][:, k] == 0xFFFF).all(), op
            j = info["never"]
        remap[k] = j
    o = enc.ops
    return columns.OpColumns(o.f.copy(), remap[o.a].astype(np.int32), o.b.copy(), o.process.copy(), o.inv_pos.copy(), o.ret_pos.copy(), o.n_events, o.n_process)


def make(model, seed, **kw):
    if model in ("mutex", "mutex-held"):
        hist = mutex_history(seed=seed, **kw)
        enc, om = encode_mutex(hist, held=model == "mutex-held")
    elif model == "table":
        hist = table_history(seed=seed, **kw)
        enc, om = encode_table(hist)
    else:
        hist = set_table_history(seed=seed, **kw)
        enc, om = encode_set_table(hist)
    return hist, enc, om


def make_case(name, model, seed, **kw):
    hist, enc, om = make(model, seed, **kw)
    if model in ("mutex", "mutex-held"):
        return Case(name, model, hist, enc.ops, enc.native_model, om), enc, om
    info = universal_table(model)
    return Case(name, model, hist, recode(enc, info), core.make_model(N.MODEL_TABLE, 0, info["table"]),
                {"kind": 3, "init": 0, "table": info["table"]}, info["states"]), enc, om


def check_shape(c, mw, crashes, own_table=None, min_ops=100):
    """what a case is named for, asserted: its mask words, that it has (no) crashed calls, that most invocations survived, its table"""
    ops = c.ops
    assert mask_words(ops) == mw, (c.name, ops.n_process)
    assert (c.crashed > 0) == crashes, (c.name, c.crashed)
    assert len(ops) >= min_ops and survived(c.hist, ops) >= 0.5, (c.name, len(ops), survived(c.hist, ops))
    assert MIN_PEAK.get(c.name.split("/")[0], 4) <= c.peak <= ops.n_process, (c.name, c.peak)
    if c.model == "mutex-held":
        assert [o["f"] for o in c.hist[:1]] == ["release"], c.name
    if c.model == "table":          # 3 accounts sharing 12: C(14, 2) = 91 states; the history's own table 40 - 110 classes, the shared one all 111
        assert own_table.shape[0] == 91 and 40 <= own_table.shape[1] <= 110 and c.om["table"].shape == (91, 111), (c.name, own_table.shape)
        assert int(ops.a.max()) >= 40 and len(np.unique(ops.a)) >= 40, c.name          # (the lookup's stride matters: classes far from 0)
    elif c.model == "set-table":
        assert len(c.hist) < 400 and 4 <= own_table.shape[0] <= 32 and c.om["table"].shape == (32, 39), (c.name, own_table.shape)


_CASES = {}


def references(oracle, names=None, seeds=SEEDS):
    """The medium cases (every shape x seeds), built once per session and shared: shape asserted, answered by the sequential oracle
    inside MAX_STEPS (asserted: nothing is left out), valid or not as the shape says -- and, for a table case, answered the same
    under the history's own table as under the shared one.  names: the shapes wanted, in the order given (default all)."""
    by_name = {s[0]: s for s in SHAPES}
    out = []
    for name in (names if names is not None else [s[0] for s in SHAPES]):
        _, model, mw, kw, crashes, bad = by_name[name]
        for seed in seeds:
            key = (name, seed)
            if key not in _CASES:
                c, enc, own = make_case(f"{name}/{seed}", model, 100 + seed, **kw)
                check_shape(c, mw, crashes, own.get("table"))
                c.ref = oracle.check(c.d(), c.om, "window", max_steps=MAX_STEPS)
                assert c.ref["valid"] != -1, (c.name, "the reference did not finish")
                assert c.ref["valid"] == (0 if bad else 1), (c.name, c.ref["valid"])
                if not c.is_mutex:
                    r = oracle.check(enc.ops.as_dict(), own, "window", max_steps=MAX_STEPS)
                    assert (r["valid"], r["fail_op"], r["steps"], r["visited"]) == (c.ref["valid"], c.ref["fail_op"], c.ref["steps"], c.ref["visited"]), c.name
                    assert r["valid"] != 1 or np.array_equal(r["witness"], c.ref["witness"]), c.name
                _CASES[key] = c
            out.append(_CASES[key])
    return out

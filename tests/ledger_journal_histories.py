"""TEST INFRASTRUCTURE.  Seeded ledger histories WITH LOOKUPS for the journal audit (jepsen/ledger.py JournalAudit), the plants its
tests share, and the shape cases of its emulator and GPU tests.

`journal_ledger` simulates workers as ledger_realtime_histories.concurrent_ledger does -- every op is invoked, takes effect at a later
step and completes at a still later one -- with :l-t lookups among the ops.  The ledger keeps a JOURNAL: the micro-ops of the transfers
applied so far, in the order they were applied.  A lookup returns the journal as it is when it takes effect, a read the counters.  A
transfer that completes :ok applies when it takes effect; one that completes :info or stays open applies then or LATE (when the workers
are done, before the final ops); one that completes :fail never applies (fail=0 by default: such a transfer is in no final lookup, which
lookup-transfers reports).  After the workers every process makes a :final? read and a :final? lookup.  The history is valid by
construction for SI, lookup-transfers, final-reads, realtime, snapshots and the journal audit.

Plants (`plant(h, meta, name)` returns a changed copy of the history):
  altered    a bit flipped in one amount, in every final lookup alike
  failed     a transfer that completed :fail journalled in every final lookup alike (needs fail > 0)
  early      a transfer journalled in a lookup that completed before the transfer was invoked
  lost       a transfer acknowledged :ok before a mid-history lookup began, and shown by no earlier lookup, dropped from that lookup
  vanished   a transfer that did not complete :ok dropped from a mid-history lookup after an earlier lookup showed it
  ahead-of-journal
             the amount of a transfer that completes :info and applies late shows in the balances of the reads before the journal has
             it: :SI's total stays, the reads stay a chain, and the extra money hides under the slack the :info transfer leaves in
             realtime's hi.  A read that completed before a lookup without the transfer began is AHEAD of that lookup.  (This stands
             where "a transfer applied twice to the balances" was asked for.  A literal second application that realtime passes needs
             an :info transfer that is never applied as slack up to the final reads, and lookup-transfers reports that transfer as
             missing from the final lookups: no history carries it past all five members.  The audit does NOT claim to catch a
             duplicated packet as such; it catches balances the journal does not explain, whatever made them.)
"""
import random

import numpy as np

PLANTS = ("altered", "failed", "early", "lost", "vanished", "ahead-of-journal")
MEMBERS = ("SI", "lookup-transfers", "final-reads", "realtime", "snapshots")
# the members of test(realtime=True, snapshots=True) on the host route that still PASS each plant
PASSES = {"altered": MEMBERS, "failed": ("SI", "final-reads", "realtime", "snapshots"),
          "early": MEMBERS, "lost": MEMBERS, "vanished": MEMBERS, "ahead-of-journal": MEMBERS}


def _entry(mop):
    return ["l-t", mop[1], dict(mop[2])]


def journal_ledger(seed, workers=4, ops=80, accounts=8, read_share=0.35, lookup_share=0.15, fail=0.0, info=0.12, open_=0.05, max_mops=3, funded=100, finals=None, kinds=None):
    """-> (history, opts, meta).  kinds: the ops' kinds in order of invocation ("r", "l" or "t"), instead of `ops` and the shares.  meta: "transfers" [{"inv", "ret", "status", "mops", "applied": step or None, "late"}], "reads" [{"inv", "ret",
    "eff"}], "lookups" [{"inv", "ret", "eff", "final"}], "late_at" the step at which the late transfers applied."""
    rng = random.Random(seed)
    ops = ops if kinds is None else len(kinds)
    accts = list(range(1, accounts + 1))
    init = {a: {"credits-posted": funded, "debits-posted": 0} for a in accts}
    cr, db = {a: funded for a in accts}, {a: 0 for a in accts}
    hist, journal, w_state, next_id, started, clock = [], [], [None] * workers, 1, 0, 0         # (journal: the entries, made once and shared by the lookups)
    process = list(range(workers))
    meta = {"transfers": [], "reads": [], "lookups": [], "late_at": None}

    def emit(p, typ, value, final=False):
        op = {"type": typ, "f": "txn", "value": value, "process": p, "index": len(hist), "time": 1000 * (len(hist) + 1)}
        if final:
            op["final?"] = True
        hist.append(op)
        return len(hist) - 1

    def apply(t):
        t["applied"] = clock
        for mop in t["mops"]:
            m = mop[2]
            cr[m["credit-acct"]] += m["amount"]; db[m["debit-acct"]] += m["amount"]
            journal.append(_entry(mop))

    snapshot = lambda: [["r", a, {"credits-posted": cr[a], "debits-posted": db[a]}] for a in accts]
    while started < ops or any(s is not None for s in w_state):
        clock += 1
        w = rng.randrange(workers)
        s = w_state[w]
        if s is None:
            if started >= ops:
                continue
            started += 1
            x = rng.random() if kinds is None else {"r": 0.0, "l": read_share, "t": 1.0}[kinds[started - 1]]
            if x < read_share:
                w_state[w] = {"kind": "r", "step": 0, "inv": emit(process[w], "invoke", [["r", a, None] for a in accts])}
            elif x < read_share + lookup_share:
                w_state[w] = {"kind": "l", "step": 0, "inv": emit(process[w], "invoke", [["l-t", None, None]])}
            else:
                mops = []
                for _ in range(rng.randint(1, max_mops)):
                    d = rng.choice(accts)
                    c = d if rng.random() < 0.1 else rng.choice(accts)
                    mops.append(["t", next_id, {"debit-acct": d, "credit-acct": c, "amount": rng.choice((0, 1, 1, 2, 3, 5))}])
                    next_id += 1
                y = rng.random()
                outcome = "fail" if y < fail else "info" if y < fail + info else "open" if y < fail + info + open_ else "ok"
                t = {"inv": emit(process[w], "invoke", mops), "ret": None, "status": outcome, "mops": mops, "applied": None,
                     "late": outcome in ("info", "open") and rng.random() < 0.5}
                meta["transfers"].append(t)
                w_state[w] = {"kind": "t", "step": 0, "t": t}
        elif s["step"] == 0:                                    # the op takes effect
            s["step"] = 1
            s["eff"] = clock
            if s["kind"] == "r":
                s["value"] = snapshot()
            elif s["kind"] == "l":
                s["value"] = list(journal) or [["l-t", None, None]]
            elif s["t"]["status"] != "fail" and not s["t"]["late"]:
                apply(s["t"])
        else:                                                   # the op completes
            w_state[w] = None
            if s["kind"] == "r":
                meta["reads"].append({"inv": s["inv"], "ret": emit(process[w], "ok", s["value"]), "eff": s["eff"]})
            elif s["kind"] == "l":
                if s["value"][0][1] is None:                    # (an empty journal has no first micro-op to tell its kind by: the lookup crashes)
                    emit(process[w], "info", s["value"])
                    process[w] += workers
                else:
                    meta["lookups"].append({"inv": s["inv"], "ret": emit(process[w], "ok", s["value"]), "eff": s["eff"], "final": False})
            elif s["t"]["status"] == "open":
                process[w] += workers
            else:
                s["t"]["ret"] = emit(process[w], s["t"]["status"], s["t"]["mops"])
                if s["t"]["status"] == "info":
                    process[w] += workers
    clock += 1
    meta["late_at"] = clock
    for t in meta["transfers"]:
        if t["late"]:
            apply(t)
    for w in range(workers if finals is None else finals):
        clock += 1
        inv = emit(process[w], "invoke", [["r", a, None] for a in accts])
        meta["reads"].append({"inv": inv, "ret": emit(process[w], "ok", snapshot(), final=True), "eff": clock})
        if journal:
            inv = emit(process[w], "invoke", [["l-t", None, None]])
            meta["lookups"].append({"inv": inv, "ret": emit(process[w], "ok", list(journal), final=True), "eff": clock, "final": True})
    opts = {"accounts": accts, "initial": init, "total-amount": funded * accounts, "negative-balances?": False}
    return hist, opts, meta


def _ids(op):
    return {m[1] for m in op["value"]}


def plant(hist, meta, name):
    """-> (the history with `name` planted, {"counts": {kind: total the plant gives}}).  Only the ops it changes are made anew (the
    entries of a generated history are shared between its lookups)."""
    h = list(hist)
    finals = [L for L in meta["lookups"] if L["final"]]
    mids = [L for L in meta["lookups"] if not L["final"]]
    ids_of = {}

    def ids_at(i):
        if i not in ids_of:
            ids_of[i] = _ids(hist[i])
        return ids_of[i]

    shown_before = lambda L, ident: any(K["ret"] < L["inv"] and ident in ids_at(K["ret"]) for K in meta["lookups"])

    def set_value(i, value):
        h[i] = dict(h[i], value=value)

    if name == "altered":
        ident = next(m[1] for m in h[finals[0]["ret"]]["value"] if m[2]["amount"] > 0)
        for L in finals:
            set_value(L["ret"], [["l-t", ident, dict(m[2], amount=m[2]["amount"] ^ 4)] if m[1] == ident else m for m in h[L["ret"]]["value"]])
        return h, {"counts": {"altered": len(finals)}}
    if name == "failed":
        t = next(t for t in meta["transfers"] if t["status"] == "fail")
        for L in finals:
            set_value(L["ret"], h[L["ret"]]["value"] + [_entry(t["mops"][0])])
        return h, {"counts": {"failed": len(finals)}}
    if name == "early":
        for L in mids:
            t = next((t for t in meta["transfers"] if t["inv"] > L["ret"]), None)
            if t is not None:
                set_value(L["ret"], h[L["ret"]]["value"] + [_entry(m) for m in t["mops"]])
                return h, {"counts": {"early": len(t["mops"])}}
    if name in ("lost", "vanished"):
        for L in reversed(mids):
            have = ids_at(L["ret"])
            for t in meta["transfers"]:
                ident = t["mops"][0][1]
                if ident not in have:
                    continue
                if name == "lost" and t["status"] == "ok" and t["ret"] < L["inv"] and not shown_before(L, ident):
                    pass
                elif name == "vanished" and t["status"] != "ok" and shown_before(L, ident):
                    pass
                else:
                    continue
                # (a later lookup is not touched: it shows the transfer again)
                set_value(L["ret"], [m for m in h[L["ret"]]["value"] if m[1] != ident])
                return h, {"counts": {name: 1}}
    if name == "ahead-of-journal":
        for t in meta["transfers"]:
            mop = next((m for m in t["mops"] if m[2]["amount"] > 0), None)
            if not (t["late"] and t["status"] == "info" and mop):
                continue
            # the reads that began after the transfer completed and took effect before it applied show its first micro-op's amount already
            window = [R for R in meta["reads"] if t["ret"] < R["inv"] and R["eff"] < meta["late_at"]]
            if not any(R["ret"] < L["inv"] and L["eff"] < meta["late_at"] for R in window for L in mids):
                continue
            extra = lambda ident, m: dict(m, **{"credits-posted": m["credits-posted"] + (mop[2]["amount"] if ident == mop[2]["credit-acct"] else 0),
                                                "debits-posted": m["debits-posted"] + (mop[2]["amount"] if ident == mop[2]["debit-acct"] else 0)})
            for R in window:
                set_value(R["ret"], [["r", ident, extra(ident, m)] for _r, ident, m in h[R["ret"]]["value"]])
            return h, {"counts": {"ahead": ">0"}}
    raise AssertionError(f"no place for the plant {name!r} in this history")


def planted(name, seed=None):
    """a history with one plant, and the seed that has a place for it"""
    for s in range(seed if seed is not None else 1, (seed if seed is not None else 1) + 40):
        h, o, meta = journal_ledger(s, workers=5, ops=140, fail=0.12 if name == "failed" else 0.0)
        try:
            hp, info = plant(h, meta, name)
        except (AssertionError, StopIteration):
            continue
        return hp, o, info["counts"]
    raise AssertionError(name)


# ---------------------------------------------------------------- what the emulator and the GPU tests both assert

def assert_same(got, want, tag):
    from jepsen_tigerbeetle_amd.jepsen import ledger as L
    for k in L.JN_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)
    assert {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")} == want["summary"], tag


def bytes_bound(cols, n_accounts):
    """what the device gets at least, and at most: 33 bytes a transfer micro-op and an entry, 25 a read micro-op, plus the head"""
    from jepsen_tigerbeetle_amd import _native as N
    from jepsen_tigerbeetle_amd.jepsen import ledger as L
    E, NL, R, M = L.journal_shapes(cols)
    rd = (cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ)
    Rm = int((cols.mop_off[1:][rd].astype(np.int64) - cols.mop_off[:-1][rd].astype(np.int64)).sum())
    columns = 33 * (M + E) + 25 * Rm
    return columns, columns + 9 * M + 20 * (NL + 1) + 16 * (R + 1) + 28 * n_accounts + 512 + 28 * 256


# ---------------------------------------------------------------- shape cases: the smallest at which the kernels can go wrong

def _op(hist, p, typ, value, final=False):
    op = {"type": typ, "f": "txn", "value": value, "process": p, "index": len(hist), "time": 1000 * (len(hist) + 1)}
    if final:
        op["final?"] = True
    hist.append(op)


def _t(ident, d, c, amount):
    return ["t", ident, None if d is None else {"debit-acct": d, "credit-acct": c, "amount": amount}]


def staged(accts, transfers, lookups, reads=2, statuses=None, init=None, bare=False, partial=False):
    """`transfers` (lists of (id, debit, credit, amount) micro-ops; debit None: a nil micro-op) invoked and completed one after the other
    (statuses[k]: "ok" "fail" "info" "open"), then `lookups` (lists of entries (id, debit, credit, amount)), each invoked and completed,
    with a read before the transfers, one after them and one after the lookups (reads = 3, 2, 1 or 0 of them).  The reads return the
    counters the ok and info transfers give.  bare: the first lookup and the first read have no invocation.  partial: the reads leave
    out the last account."""
    init = init or {}
    cr = {a: init.get(a, {}).get("credits-posted", 0) for a in accts}
    db = {a: init.get(a, {}).get("debits-posted", 0) for a in accts}
    hist = []
    n_read = [0]

    def read(p):
        ids = accts[:-1] if partial and len(accts) > 1 else accts
        if not (bare and n_read[0] == 0):
            _op(hist, p, "invoke", [["r", a, None] for a in ids])
        n_read[0] += 1
        _op(hist, p, "ok", [["r", a, {"credits-posted": cr[a], "debits-posted": db[a]}] for a in ids])

    if reads >= 3:
        read(0)
    statuses = statuses or ["ok"] * len(transfers)
    for k, (mops, status) in enumerate(zip(transfers, statuses)):
        v = [_t(*m) for m in mops]
        _op(hist, 10 + k, "invoke", v)
        if status in ("ok", "info"):
            for _i, d, c, amount in mops:
                if d is not None:
                    if c in cr: cr[c] += amount
                    if d in db: db[d] += amount
        if status != "open":
            _op(hist, 10 + k, status, v)
    if reads >= 2:
        read(1)
    for k, entries in enumerate(lookups):
        if not (bare and k == 0):
            _op(hist, 1000 + k, "invoke", [["l-t", None, None]])
        _op(hist, 1000 + k, "ok", [["l-t", i, None if d is None else {"debit-acct": d, "credit-acct": c, "amount": a}] for i, d, c, a in entries], final=k + 2 >= len(lookups))
    if reads >= 1:
        read(2)
    return hist, {"accounts": list(accts), "initial": init}


def shape_cases(big=True, slice_entries=4096, chunk=256, window_words=8192, grid_cap=2048):
    """[{"name", "history", "opts", "counts": {summary field or kind: the value the case was built for}}].  big=False leaves out the cases
    sized by the library's own constants (the emulator reaches those paths with small plan knobs); slice_entries, chunk, window_words,
    grid_cap: the plan's and the launch sequence's constants the sizes are taken from."""
    rng = random.Random(9)
    cases = []

    def add(name, hist_opts, **counts):
        h, o = hist_opts
        cases.append({"name": name, "history": h, "opts": o, "counts": counts})

    A8 = list(range(1, 9))
    xf = lambda n, accts=A8, first=1: [[(first + k, rng.choice(accts), rng.choice(accts), rng.randint(0, 9))] for k in range(n)]
    flat = lambda ts: [m for t in ts for m in t]
    T5 = xf(5)
    add("no-lookups", staged(A8, T5, []), n_lookups=0, n_records=5, n_checked=16)
    add("no-transfers", staged(A8, [], [[(1, 1, 2, 3)], [(2, 1, 2, 3), (2, 1, 2, 3)]]), n_xfer_mops=0, unknown=3, n_entries=3)
    add("no-reads", staged(A8, T5, [flat(T5)], reads=0), read_count=0, n_entries=5, n_checked=0)
    add("one-entry", staged(A8, T5, [flat(T5)[:1]]), n_entries=1, lost=4)
    for n in (63, 64, 65, 255, 256, 257):
        T = xf(n)
        add(f"{n}-entries", staged(A8, T, [flat(T)]), n_entries=n, n_records=n, lost=0)
    for n in (31, 32, 33):
        T = xf(n)
        add(f"{n}-records", staged(A8, T, [flat(T)[::2], flat(T)]), n_records=n, lost=n // 2, vanished=0)
    T = xf(40)
    add("two-lookups-vanished", staged(A8, T, [flat(T), flat(T)[:30], flat(T)]), vanished=10, lost=10)
    T = xf(12)
    add("65-lookups", staged(A8, T, [flat(T)[:k % 13] or flat(T)[:1] for k in range(65)]), n_lookups=65)
    add("only-unknown-ids", staged(A8, T5, [[(100 + k, 1, 2, 3) for k in range(70)]]), unknown=70, lost=5)
    add("every-entry-repeated", staged(A8, T5, [flat(T5) * 3]), repeated=10, altered=0)
    add("reinvoked-with-other-fields", staged(A8, [[(1, 1, 2, 3)], [(1, 2, 3, 4)], [(2, 3, 4, 5), (2, 3, 4, 6)]], [[(1, 1, 2, 3), (2, 3, 4, 5)], [(1, 2, 3, 4), (2, 3, 4, 6)]]),
        n_records=2, n_reinvoked=2, altered=2)
    add("nil-entries-and-nil-records", staged(A8, [[(1, None, None, None)], [(2, 1, 2, 3)], [(3, 2, 3, 4)]], [[(1, None, None, None), (2, None, None, None), (3, 2, 3, 4)]] * 2),
        altered=4, foreign_sides=2)
    add("foreign-sides", staged(A8, [[(1, 1, 99, 3)], [(2, 98, 2, 4)], [(3, 97, 96, 5)], [(4, 3, 4, 6)]], [[(1, 1, 99, 3), (2, 98, 2, 4), (3, 97, 96, 5), (4, 3, 4, 6)]]), foreign_sides=4, altered=0)
    T = xf(8)
    add("ok-fail-info-open", staged(A8, T, [flat(T)[:6], flat(T)[2:]], statuses=["ok", "fail", "info", "open"] * 2), failed=3, lost=1, vanished=2)
    add("lookup-and-read-without-invocation", staged(A8, T5, [flat(T5)[:3], flat(T5)], bare=True), lost=0, n_lookups=2)
    T = xf(9, [7])
    add("one-account", staged([7], T, [flat(T)]), n_checked=2, lost=0)
    A33 = list(range(100, 133))
    T = xf(50, A33)
    add("33-accounts", staged(A33, T, [flat(T)[:25], flat(T)]), n_checked=66, lost=25)
    A1025 = list(range(1, 2051, 2))
    T = xf(40, A1025)
    add("1025-accounts", staged(A1025, T, [flat(T)], reads=2), n_checked=2050, lost=0)
    for n in (63, 64, 65):
        h, o = staged(A8, T5, [flat(T5)], reads=1)
        last = h[-2:]
        for k in range(n - 1):
            for op in last:
                h.append(dict(op, process=2000 + k, index=len(h)))
        add(f"{n}-reads", (h, o), read_count=n, n_checked=8 * n)
    add("partial-reads", staged(A8, T5, [flat(T5)], partial=True), n_checked=14)
    add("amounts-0-and-2^31-1", staged(A8, [[(1, 1, 2, 0)], [(2, 2, 3, 2 ** 31 - 1)], [(3, 2, 3, 2 ** 31 - 1)]], [[(1, 1, 2, 0), (2, 2, 3, 2 ** 31 - 1), (3, 2, 3, 2 ** 31 - 1)]]), altered=0, lost=0)
    # reads ahead of and behind the books: a lookup that lacks an applied transfer, and one that has a transfer the reads do not show
    h, o = staged(A8, [[(1, 1, 2, 5)], [(2, 3, 4, 7)]], [[(1, 1, 2, 5)], [(1, 1, 2, 5), (2, 3, 4, 7)]], reads=3, statuses=["ok", "open"])
    add("ahead-and-behind", (h, o), lost=0)
    for name in PLANTS:
        hp, o, counts = planted(name)
        add("planted-" + name, (hp, o), **{k: v for k, v in counts.items()})
    h, o, _meta = journal_ledger(3, workers=6, ops=200)
    add("valid-concurrent", (h, o), valid=1)
    if big:
        n = 32 * window_words + 1                               # one record past the LDS window
        T = [[(k + 1, 1 + k % 8, 1 + (k // 8) % 8, k % 5) for k in range(n)]]           # (one transfer of n micro-ops)
        add("one-record-past-the-window", staged(A8, T, [flat(T)[-3:], flat(T)[::1000] + flat(T)[-2:]]), n_records=n)
        T = xf(chunk + 1)
        add("one-record-past-a-chunk", staged(A8, T, [flat(T)]), n_records=chunk + 1, lost=0)
        T = xf(300)
        add("one-entry-past-a-slice", staged(A8, T, [(flat(T) * (slice_entries // 300 + 1))[:slice_entries + 1]]), n_entries=slice_entries + 1)
        # more work than the grids of the strided kernels (grid_cap workgroups): every one of them takes a second trip on the device
        n = 4 * grid_cap + 1                                    # reads: a wavefront each, four to a workgroup
        T = xf(9)
        h, o = staged(A8, T, [flat(T)[:4], flat(T)], reads=3)
        last = h[-2:]
        for k in range(n - 3):
            for op in last:
                h.append(dict(op, process=2000 + k, index=len(h)))
        add("more-reads-than-the-grid", (h, o), read_count=n, n_checked=8 * n)
        n = grid_cap * chunk + 1                                # transfer micro-ops: 256 a workgroup of the table's kernels, a chunk a workgroup of the members
        T = [[(k + 1, 1 + k % 8, 1 + (k // 8) % 8, k % 5) for k in range(n)]]           # (one transfer of n micro-ops)
        add("more-chunks-than-the-grid", staged(A8, T, [flat(T)[-300:], flat(T)[::997] + flat(T)[-2:], flat(T)[:5]]), n_records=n, n_lookups=3)
        n = grid_cap + 1                                        # slices: every lookup has one of its own at least
        T = xf(12)
        add("more-slices-than-the-grid", staged(A8, T, [flat(T)[k % 5:k % 5 + 1 + k % 7] for k in range(n)]), n_lookups=n)
    assert [c["name"] for c in cases] == shape_case_names(big)
    return cases


def shape_case_names(big=True):
    """the names of shape_cases(big), without building a history (a test file parametrises by them and builds the cases in a fixture)"""
    names = ["no-lookups", "no-transfers", "no-reads", "one-entry"] + [f"{n}-entries" for n in (63, 64, 65, 255, 256, 257)]
    names += [f"{n}-records" for n in (31, 32, 33)] + ["two-lookups-vanished", "65-lookups", "only-unknown-ids", "every-entry-repeated",
              "reinvoked-with-other-fields", "nil-entries-and-nil-records", "foreign-sides", "ok-fail-info-open", "lookup-and-read-without-invocation",
              "one-account", "33-accounts", "1025-accounts"] + [f"{n}-reads" for n in (63, 64, 65)]
    names += ["partial-reads", "amounts-0-and-2^31-1", "ahead-and-behind"] + ["planted-" + p for p in PLANTS] + ["valid-concurrent"]
    if big:
        names += ["one-record-past-the-window", "one-record-past-a-chunk", "one-entry-past-a-slice", "more-reads-than-the-grid",
                  "more-chunks-than-the-grid", "more-slices-than-the-grid"]
    return names

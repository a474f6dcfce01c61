"""Seeded generators of ledger histories (the ops `edn.read_history` gives for the reference's ledger workload) for the ledger tests:
`Builder` writes ops one by one (the shape tests lay out reads, transfers and final rows exactly), `random_ledger` simulates workers
over funded accounts and plants anomalies by name.  Accounts start with `funds` credits each, so a valid history has
total-amount = funds x accounts and no negative balance."""
import random

ANOMALIES = ("wrong-total", "negative", "unexpected", "nil", "dup-id", "missing-transfer", "final-read-field", "final-read-order",
             "final-read-length", "final-lookup-field", "final-lookup-order", "final-lookup-length", "no-final")


def r_mop(ident, credits, debits=0):
    return ["r", ident, {"credits-posted": credits, "debits-posted": debits}]


def t_mop(f, ident, debit, credit, amount):
    return [f, ident, {"debit-acct": debit, "credit-acct": credit, "amount": amount}]


class Builder:
    def __init__(self):
        self.h = []
        self.time = 0

    def op(self, type_, value, process, final=False):
        self.time += 1000
        o = {"type": type_, "f": "txn", "value": value, "process": process, "index": len(self.h), "time": self.time}
        if final:
            o["final?"] = True
        self.h.append(o)
        return o

    def nemesis(self):
        self.time += 1000
        self.h.append({"type": "info", "f": "kill", "value": None, "process": "nemesis", "index": len(self.h), "time": self.time})

    def transfer(self, ident, debit=1, credit=2, amount=1, process=0, complete="ok"):
        v = [t_mop("t", ident, debit, credit, amount)]
        self.op("invoke", v, process)
        if complete:
            self.op(complete, v, process)

    def read(self, mops, process=0, final=False, complete="ok"):
        """mops: [["r", id, {...} | None], ...] as the completion returns them"""
        self.op("invoke", [["r", m[1], None] for m in mops] or [["r", 1, None]], process, final)
        if complete:
            self.op(complete, mops if complete == "ok" else [["r", m[1], None] for m in mops], process, final)

    def lookup(self, transfers, process=0, final=True, complete="ok"):
        """transfers: [(id, debit, credit, amount), ...] as the completion returns them"""
        self.op("invoke", [["l-t", None, None]], process, final)
        if complete:
            self.op(complete, [t_mop("l-t", *t) for t in transfers] if complete == "ok" else [["l-t", None, None]], process, final)


def balanced(ids, total, rng=None, big=0):
    """read micro-ops over `ids` whose balances sum to `total`, none negative (total >= 0); with `big`, credits and debits of that size
    on the first id (the balance unchanged)"""
    n = len(ids)
    if abs(total) >= 2 ** 40:                                  # (a huge total sits on the first id: the others stay small)
        share, rest = 1000, total - 1000 * n
    else:
        share, rest = divmod(total, n)
    out = []
    for k, ident in enumerate(ids):
        bal = share + (rest if k == 0 else 0)
        debits = (rng.randrange(0, 50) if rng else 0) + (big if k == 0 else 0)
        out.append(r_mop(ident, bal + debits, debits))
    return out


def random_ledger(seed, workers=4, accounts=range(1, 9), transfers=30, reads=20, info=0.0, fail=0.0, final=True, funds=100, plant=()):
    """-> (history, opts).  Workers take turns at random; a transfer moves 1..5 from an account that has it; an :info transfer is
    applied or not at random, a :fail one is not.  A read returns every account.  The final phase: every worker a :final? read, then
    every worker a :final? lookup of all applied transfers.  plant: names of ANOMALIES."""
    rng = random.Random(seed)
    accounts = list(accounts)
    plant = set(plant)
    assert plant <= set(ANOMALIES), plant - set(ANOMALIES)
    cr = {a: funds for a in accounts}
    db = {a: 0 for a in accounts}
    b = Builder()
    applied = []
    kinds = ["t"] * transfers + ["r"] * reads
    rng.shuffle(kinds)
    read_no, next_id = 0, 1
    targets = {name: rng.randrange(max(1, reads)) for name in ("wrong-total", "negative", "unexpected", "nil", "dup-id")}
    state = lambda: [r_mop(a, cr[a], db[a]) for a in accounts]
    for n, kind in enumerate(kinds):
        p = rng.randrange(workers)
        if n % 17 == 5:
            b.nemesis()
        roll = rng.random()
        complete = "info" if roll < info else "fail" if roll < info + fail else "ok"
        if kind == "t":
            d = rng.choice([a for a in accounts if cr[a] - db[a] >= 5] or accounts)
            c = rng.choice([a for a in accounts if a != d] or accounts)
            amt = rng.randint(1, 5)
            if complete == "ok" or (complete == "info" and rng.random() < 0.5):
                db[d] += amt; cr[c] += amt
                applied.append((next_id, d, c, amt))
            b.transfer(next_id, d, c, amt, p, complete)
            next_id += 1
            continue
        mops = state()
        hit = {name for name in plant if targets.get(name) == read_no}
        if "wrong-total" in hit:
            mops[0][2]["credits-posted"] += 3
        if "negative" in hit and len(accounts) > 1:
            x = mops[0][2]["credits-posted"] - mops[0][2]["debits-posted"] + 4
            mops[0][2]["debits-posted"] += x; mops[1][2]["credits-posted"] += x
        if "unexpected" in hit:
            mops.append(r_mop(max(accounts) + 1000, 7, 7))
        if "nil" in hit:
            mops[-1][2] = None
        if "dup-id" in hit:
            mops.insert(0, r_mop(mops[-1][1], 12345, 0))          # (the later micro-op of that id wins)
        b.read(mops, p, complete=complete)
        read_no += 1
    if final and "no-final" not in plant:
        for w in range(workers):
            mops = state()
            if w == workers - 1 and workers > 1:
                if "final-read-field" in plant:
                    mops[-1][2]["credits-posted"] += 1; mops[-1][2]["debits-posted"] += 1
                if "final-read-order" in plant and len(mops) > 1:
                    mops[0], mops[1] = mops[1], mops[0]
                if "final-read-length" in plant:
                    mops.append(r_mop(accounts[0] + 500, 0, 0))
            b.read(mops, w, final=True)
        for w in range(workers):
            rows = list(applied)
            if w == 0 and "missing-transfer" in plant and rows:
                del rows[len(rows) // 2]
            if w == workers - 1 and workers > 1 and rows:
                if "final-lookup-field" in plant:
                    i, d, c, amt = rows[-1]
                    rows[-1] = (i, d, c, amt + 1)
                if "final-lookup-order" in plant and len(rows) > 1:
                    rows[0], rows[1] = rows[1], rows[0]
                if "final-lookup-length" in plant:
                    rows.append(rows[0])
            b.lookup(rows, w)
    return b.h, {"accounts": accounts, "total-amount": funds * len(accounts), "negative-balances?": False}


def expected(history, opts):
    """What tbc_ledger_check must return for `history` -- every output array and every summary field -- worked out with the host statement's
    own functions (jepsen/ledger.py check_op, err_badness, max-by / min-by), and held against the result maps of its checkers."""
    import numpy as np
    from jepsen_tigerbeetle_amd import _native as N
    from jepsen_tigerbeetle_amd.jepsen import ledger as L
    accounts, total, neg = L._si_opts(None, opts)
    accts = set(accounts)
    client = [op for op in L._indexed(history) if L.H.client_op(op)]
    reads = [L._bank_op(op) for op in client if op["type"] == "ok" and L.op_txn_f(op) == "r"]
    errs = [L.check_op(accts, total, neg, op) for op in reads]
    code = [L.ERROR_TYPES.index(e["type"]) if e else 0 for e in errs]
    bad = [L.err_badness(total, e) if e else 0 for e in errs]
    out = {"read_error": np.array(code, np.uint8), "read_badness": np.array(bad, np.int64),
           "read_total": np.array([sum(b for b in op["value"].values() if b is not None) for op in reads], np.int64)}
    none = N.NO_OP
    totals = out["read_total"].tolist()
    s = {"read_count": len(reads), "error_count": sum(1 for c in code if c), "first_error": next((r for r, c in enumerate(code) if c), none), "errors": {}}
    for k in range(1, 5):
        rs = [r for r, c in enumerate(code) if c == k]
        s["errors"][L.ERROR_TYPES[k]] = {"count": len(rs), "first": rs[0] if rs else none, "last": rs[-1] if rs else none,
                                         "worst": L._max_by(lambda r: bad[r], rs) if rs else none}
    rs = [r for r, c in enumerate(code) if c == 3]
    s["lowest"] = L._min_by(lambda r: totals[r], rs) if rs else none
    s["highest"] = L._max_by(lambda r: totals[r], rs) if rs else none
    T = set()
    for op in client:
        if op["type"] == "invoke" and L.op_txn_f(op) == "t":
            T.update(m[1] for m in op["value"])
    fr, fl = L._final_rows(history, "r"), L._final_rows(history, "l-t")
    out["lookup_missing"] = np.array([len(T - {m[1] for m in op["value"]}) for op in fl], np.uint32)
    # (a :final? read's value as the columns hold it: its vector; the generators plant no repeated id in a final read)
    out["final_read_unlike"] = np.array([op["value"] != fr[0]["value"] for op in fr], np.uint8)
    out["final_lookup_unlike"] = np.array([op["value"] != fl[0]["value"] for op in fl], np.uint8)
    s.update({"n_transfers": len(T), "n_final_reads": len(fr), "final_reads_unlike": int(out["final_read_unlike"].sum()), "n_final_lookups": len(fl),
              "final_lookups_unlike": int(out["final_lookup_unlike"].sum()), "suspect_lookups": int((out["lookup_missing"] != 0).sum())})
    s["valid_si"], s["valid_lookups"] = int(s["error_count"] == 0), int(s["suspect_lookups"] == 0)
    s["valid_final_reads"] = int(len(fr) >= 1 and len(fl) >= 1 and not s["final_reads_unlike"] and not s["final_lookups_unlike"])
    # ---- the checkers' own maps say the same
    si = L.BankChecker(opts).check(opts, history)
    assert (si["valid?"], si["read-count"], si["error-count"]) == (bool(s["valid_si"]), s["read_count"], s["error_count"])
    assert {t: e["count"] for t, e in si["errors"].items()} == {t: e["count"] for t, e in s["errors"].items() if e["count"]}
    for t, e in si["errors"].items():
        for f in ("first", "last", "worst"):
            assert e[f]["op"] == reads[s["errors"][t][f]], (t, f)
    if "wrong-total" in si["errors"]:
        assert si["errors"]["wrong-total"]["lowest"]["op"] == reads[s["lowest"]] and si["errors"]["wrong-total"]["highest"]["op"] == reads[s["highest"]]
    lt = L.LookupAllInvokedTransfers().check(opts, history)
    assert lt["valid?"] == bool(s["valid_lookups"]) and len(lt.get("suspect-final-lookups", [])) == s["suspect_lookups"]
    assert L.FinalReads().check(opts, history)["valid?"] == bool(s["valid_final_reads"])
    out["summary"] = s
    return out


def assert_same(got, want, ctx=""):
    """tbc_ledger_check's (or the emulator's) arrays and summary against `expected`"""
    import numpy as np
    for f in ("read_error", "read_total", "read_badness", "lookup_missing", "final_read_unlike", "final_lookup_unlike"):
        assert np.array_equal(got[f], want[f]), (ctx, f, got[f].tolist()[:20], want[f].tolist()[:20])
    g = {k: v for k, v in got["summary"].items() if k not in ("ns_device", "bytes_in")}
    assert g == want["summary"], (ctx, g, want["summary"])


def transfer_row(ident):
    return (ident, 1 + ident % 7, 8, 1 + ident % 5)


def shape_ledger(seed, read_sizes, accounts=range(1, 9), n_transfers=10, n_final_reads=2, n_final_lookups=2, total=800, error_rate=0.1,
                 variant=None, missing=None, repeats=False, foreign=False, big=0, ok_rate=0.9):
    """-> (history, opts): a ledger laid out by shape.  read_sizes: the micro-ops of each read, in order (a read of n micro-ops
    reads the first n accounts, and ids that are no account beyond them); ok_rate of the reads complete :ok, the others :info (1.0:
    every read is an :ok read); transfers with ids 1000 + 3 i are invoked between the reads, a few left open or failed; about
    error_rate of the reads carry one planted error.  The final phase: n_final_reads equal reads of the first (at most 8) accounts
    and n_final_lookups lookups of every transfer; `variant` changes the LAST final read and the LAST final lookup -- "last" (the
    last micro-op), "field" (one field of a middle one), "nil" (the NIL flag only), "order", "length"; missing = {lookup number:
    positions left out}; repeats: the second half of every lookup lists its first id again; foreign: every lookup also lists ids
    nobody invoked; big: credits and debits of that size in every read (balances unchanged)."""
    rng = random.Random(seed)
    accounts = list(accounts)
    b = Builder()
    ids = [1000 + 3 * i for i in range(n_transfers)]
    n_reads = len(read_sizes)
    at = sorted(rng.randrange(n_reads + 1) for _ in ids)                   # the read each transfer comes before
    k = 0
    for r in range(n_reads + 1):
        while k < len(ids) and at[k] == r:
            b.transfer(*transfer_row(ids[k]), process=k % 5, complete=("ok", "ok", "ok", "info", "fail", None)[rng.randrange(6)])
            k += 1
        if r == n_reads:
            break
        n = read_sizes[r]
        names = accounts[:n] + [10 ** 6 + j for j in range(n - len(accounts))]
        mops = balanced(names, total, rng, big)
        if rng.random() < error_rate:
            what = rng.randrange(5)
            m = mops[rng.randrange(n)]
            if what == 0:
                m[2]["credits-posted"] += rng.choice((-2, 1, 1, 5))
            elif what == 1 and n > 1:
                x = mops[-1][2]["credits-posted"] - mops[-1][2]["debits-posted"] + rng.choice((1, 1, 9))
                mops[-1][2]["debits-posted"] += x; mops[-2][2]["credits-posted"] += x
            elif what == 2:
                m[2] = None
            elif what == 3:
                m[1] = 2 * 10 ** 6 + r
            else:
                m[2]["credits-posted"] += 7; mops[0][2] = None
        b.read(mops, process=r % 5, complete="ok" if rng.random() < ok_rate else "info")
        if r % 29 == 3:
            b.nemesis()

    def vary(rows, is_read):
        rows = [list(m[:2]) + [dict(m[2]) if m[2] else None] for m in rows]
        mid = len(rows) // 2
        if variant == "last":
            rows[-1][2]["debits-posted" if is_read else "amount"] += 1
        elif variant == "field":
            rows[mid][2]["credits-posted" if is_read else "credit-acct"] += 1
        elif variant == "nil":
            rows[mid][2] = None
        elif variant == "order" and len(rows) > 1:
            rows[0], rows[-1] = rows[-1], rows[0]
        elif variant == "length":
            rows = rows[:-1] if len(rows) > 1 else rows + [[rows[0][0], rows[0][1] + 1, rows[0][2]]]
        return rows

    fin = balanced(accounts[:8], total, None, big)
    for w in range(n_final_reads):
        b.read(vary(fin, True) if variant and w == n_final_reads - 1 and w else fin, process=w % 5, final=True)
    full = [t_mop("l-t", *transfer_row(i)) for i in ids]
    for w in range(n_final_lookups):
        rows = [m for j, m in enumerate(full) if j not in (missing or {}).get(w, ())]
        if repeats and rows:
            rows = rows[:len(rows) // 2] + [rows[0]] + rows[len(rows) // 2:] + [rows[0]]
        if foreign:
            rows = [t_mop("l-t", 5, 1, 2, 1)] + rows + [t_mop("l-t", 999999, 1, 2, 1)]
        if variant and w == n_final_lookups - 1 and w and rows:
            rows = vary(rows, False)
        b.op("invoke", [["l-t", None, None]], w % 5, True)
        b.op("ok", rows, w % 5, True)
    return b.h, {"accounts": accounts, "total-amount": total, "negative-balances?": False}


VARIANTS = ("last", "field", "nil", "order", "length")


def shape_cases():
    """[{"name", "history", "opts", and what the case promises: "ok_reads" (how many :ok reads reach the check), "runs" (how many runs
    the plan cuts them into), "variant" (how its last final read and lookup differ from the first), "final_lookups"}]: the smallest
    shapes at which each kernel of tbc_ledger_check can go wrong (tests/test_ledger_gpu.py lists them; tests/test_ledger_emu.py runs
    the same under the emulator, whose lookup window is 8 words = 256 transfers).  `references` holds every promise to the history."""
    out = []
    Ts = (0, 1, 31, 32, 33, 255, 256, 257)
    FLs = (0, 1, 2, 70)
    variants = (None,) + VARIANTS
    unsorted = lambda n: [((7 * k) % n) * 3 + 1 for k in range(n)] if n % 7 else list(range(3 * n, 0, -3))

    def add(name, read_sizes, promise=None, **kw):
        k = len(out)                                                        # (what a case does not set goes round by its number)
        kw.setdefault("n_transfers", Ts[k % len(Ts)])
        kw.setdefault("n_final_lookups", FLs[k // 2 % len(FLs)])
        kw.setdefault("variant", variants[k % len(variants)])
        kw.setdefault("repeats", k % 3 == 0)
        kw.setdefault("foreign", k % 4 == 1)
        T = kw["n_transfers"]
        if "missing" not in kw and T > 1 and k % 2 == 0 and kw["n_final_lookups"] > 1:
            kw["missing"] = {1: [0, T - 1], kw["n_final_lookups"] - 1: [T // 2]}
        h, o = shape_ledger(100 + k, read_sizes, **kw)
        out.append(dict(promise or {}, name=f"{name} T={T} FL={kw['n_final_lookups']} {kw['variant']}", history=h, opts=o))

    # exactly n :ok reads reach the check (every read :ok, no final read): the tails of the thread-per-read phases at the wavefront's
    # and the workgroup's edges; of 8 micro-ops, 32 reads a run; of one micro-op, 256 reads a run
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        add(f"reads={n}", [8] * n, {"ok_reads": n, "runs": (n + 31) // 32}, ok_rate=1.0, n_final_reads=0)
    for n in (64, 255, 256, 257, 513):
        add(f"reads={n}x1", [1] * n, {"ok_reads": n, "runs": (n + 255) // 256}, accounts=[5], ok_rate=1.0, n_final_reads=0)
    add("reads=254 and 2 final", [8] * 254, {"ok_reads": 256, "runs": 8}, ok_rate=1.0, n_final_reads=2)
    acc320 = unsorted(320)
    add("mops=63..65", [63, 64, 65] * 4 + [65, 63], accounts=acc320)
    add("one read of 300 among short ones", [8] * 40 + [300] + [8] * 40 + [3], accounts=acc320, error_rate=0.2)
    add("a read of 300 with a planted error", [300, 300, 300, 300, 300, 300], accounts=acc320, error_rate=0.7)
    rng = random.Random(9)
    add("reads straddling runs", [rng.choice((1, 2, 8, 30, 100, 128, 129, 255, 256, 257)) for _ in range(60)], accounts=acc320, error_rate=0.25)
    for n in (1, 8, 70):                                                    # accounts, handed over unsorted
        add(f"accounts={n}", [min(n, 8)] * 40 + [n] * 3 + [n + 2] * 2, accounts=unsorted(n), error_rate=0.2)
    add("more accounts than LDS holds", [8] * 20 + [1100, 7], accounts=unsorted(1100), error_rate=0.3, n_final_reads=3)
    for T in Ts:                                                            # transfers, with two and with seventy lookups
        FL = 2 if T % 2 else 70                                             # (nobody invoked anything: the lookups list strangers only)
        add(f"transfers={T}", [8] * 10, {"final_lookups": FL}, n_transfers=T, n_final_lookups=FL, missing={1: [0, T - 1]} if T > 1 else None,
            foreign=True if T == 0 else T % 4 == 1)
    for v in variants:                                                      # final rows that differ from the first
        add(f"final rows: {v}", [8] * 5, {"variant": v, "final_lookups": 5}, n_transfers=40, n_final_reads=5, n_final_lookups=5, variant=v,
            error_rate=0.0, missing={})
    add("fully valid", [8] * 70, n_transfers=300, n_final_reads=8, n_final_lookups=8, variant=None, error_rate=0.0, missing={}, repeats=False, foreign=False)
    add("no final rows", [8] * 12, n_final_reads=0, n_final_lookups=0, variant=None)
    add("final reads only", [8] * 12, n_final_reads=2, n_final_lookups=0, variant=None)
    add("repeats and strangers", [8] * 5, n_transfers=100, n_final_lookups=3, repeats=True, foreign=True, variant=None, missing={2: [7]})
    big = 2 ** 62 - 10 ** 6                                                 # totals near +-2^62, total-amount far from 0
    add("total near 2^62", [8] * 70, total=big, error_rate=0.3)
    add("total near -2^62", [8] * 70, total=-big, error_rate=0.6)
    add("big credits and debits", [8] * 70, total=12345, big=2 ** 58 - 1, error_rate=0.3)
    return out


def row_difference(first, row):
    """How a final row differs from the first: None, or (kind, positions) with kind "length", "order" (the same micro-ops in another
    order), "nil" (only maps that are nil in one and not in the other), "field" (anything else), and the positions that differ."""
    from jepsen_tigerbeetle_amd.jepsen.edn import _hashable
    if row == first:
        return None
    if len(row) != len(first):
        return ("length", [])
    at = [i for i, (x, y) in enumerate(zip(first, row)) if x != y]
    if sorted(map(_hashable, row), key=repr) == sorted(map(_hashable, first), key=repr):
        return ("order", at)
    if all(first[i][:2] == row[i][:2] and (first[i][2] is None) != (row[i][2] is None) for i in at):
        return ("nil", at)
    return ("field", at)


def landed(history, summary):
    """The names of ANOMALIES (and "valid") that `history` really holds, from the history itself and the host statement's summary of it
    (`expected`): what a randomised test asserts before it trusts its inputs."""
    from jepsen_tigerbeetle_amd.jepsen import ledger as L
    got = set()
    for name, t in (("wrong-total", "wrong-total"), ("negative", "negative-value"), ("unexpected", "unexpected-key"), ("nil", "nil-balance")):
        if summary["errors"][t]["count"]:
            got.add(name)
    for op in history:
        if L.H.client_op(op) and op["type"] == "ok" and L.op_txn_f(op) == "r" and len({m[1] for m in op["value"]}) < len(op["value"]):
            got.add("dup-id")
    if summary["suspect_lookups"]:
        got.add("missing-transfer")
    for what, f in (("final-read", "r"), ("final-lookup", "l-t")):
        rows = L._final_rows(history, f)
        for op in rows[1:]:
            d = row_difference(rows[0]["value"], op["value"])
            if d:
                got.add(f"{what}-{'field' if d[0] == 'nil' else d[0]}")
    if not summary["n_final_reads"] and not summary["n_final_lookups"]:
        got.add("no-final")
    if summary["valid_si"] and summary["valid_lookups"] and summary["valid_final_reads"]:
        got.add("valid")
    return got


# what the shape cases must cover between them, besides the promises each makes: every error type, a suspect lookup, no final rows,
# a fully valid input, and each way a final read / lookup can differ
SHAPES_COVER = {"wrong-total", "negative", "unexpected", "nil", "missing-transfer", "no-final", "valid"}


def references(cases):
    """{(name, negative_balances): (history, opts, expected)} for both ways of negative-balances?, computed once.  It asserts first that
    the cases are not vacuous, by the HOST statement's results: each case keeps its promises (how many :ok reads and final lookups it
    has, how its last final rows differ), every anomaly kind occurs in some input, and some input is fully valid."""
    from jepsen_tigerbeetle_amd.jepsen import ledger as L
    refs, seen = {}, set()
    for c in cases:
        h, o = c["history"], c["opts"]
        for neg in (False, True):
            o2 = dict(o, **{"negative-balances?": neg})
            refs[(c["name"], neg)] = (h, o2, expected(h, o2))
        s = refs[(c["name"], False)][2]["summary"]
        seen |= landed(h, s)
        if "ok_reads" in c:
            assert s["read_count"] == c["ok_reads"], (c["name"], s["read_count"])
        if "final_lookups" in c:
            assert s["n_final_lookups"] == c["final_lookups"], (c["name"], s["n_final_lookups"])
        if c.get("variant"):
            for f in ("r", "l-t"):
                rows = [op["value"] for op in L._final_rows(h, f)]
                assert all(r == rows[0] for r in rows[:-1]), c["name"]
                kind, at = row_difference(rows[0], rows[-1])
                want = {"last": ("field", [len(rows[0]) - 1]), "field": ("field", [len(rows[0]) // 2]), "nil": ("nil", [len(rows[0]) // 2]),
                        "order": ("order", [0, len(rows[0]) - 1]), "length": ("length", [])}[c["variant"]]
                assert (kind, at) == want, (c["name"], f, kind, at)
    assert not SHAPES_COVER - seen, f"no input covers {SHAPES_COVER - seen}"
    return refs

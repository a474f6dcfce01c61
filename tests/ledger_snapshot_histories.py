"""TEST INFRASTRUCTURE.  Histories for the snapshot-order checker (jepsen/ledger.py SnapshotOrder), and the shape cases its emulator and
GPU tests share.

`reads_ledger` turns a list of read values into a history of reads alone (skew does not depend on time).  Two planted anomalies on
valid concurrent ledgers (ledger_realtime_histories.concurrent_ledger):
  fork   appended to a ledger whose transfers all completed (:ok or :fail), so that its final counters are known: two :ok transfers on
         disjoint account pairs, open across two reads; R shows the first transfer only and R' the second only.  The total is intact
         and all four ops are concurrent, so :SI and the realtime bounds pass; R and R' are skewed.
  torn   one read takes half its accounts from a later read's true snapshot, the half chosen so that the total still holds and the
         torn read is skewed with some read between the two.
"""
import random

import ledger_realtime_histories as G

FIELDS = G.FIELDS
NIL = "nil"


def _op(hist, p, typ, value):
    hist.append({"type": typ, "f": "txn", "value": value, "process": p, "index": len(hist), "time": 1000 * (len(hist) + 1)})


def reads_ledger(accounts, rows, transfers_first=0):
    """rows: per read a list of (id, credits, debits) or (id, NIL); every read invoked and completed :ok in turn by one of five processes.
    transfers_first: that many :ok transfers (amount 0) before the reads, so that the columns hold micro-ops that are no read's."""
    hist = []
    for k in range(transfers_first):
        v = [["t", k + 1, {"debit-acct": accounts[0], "credit-acct": accounts[-1], "amount": 0}]]
        _op(hist, 9, "invoke", v)
        _op(hist, 9, "ok", v)
    for k, row in enumerate(rows):
        _op(hist, k % 5, "invoke", [["r", m[0], None] for m in row])
        _op(hist, k % 5, "ok", [["r", m[0], None if m[1] is NIL else {"credits-posted": m[1], "debits-posted": m[2]}] for m in row])
    return hist, {"accounts": list(accounts)}


def random_rows(rng, accounts, n):
    """reads with few distinct values (so that sums tie and reads repeat), negative ones among them, some partial"""
    rows = []
    for _ in range(n):
        row = [(a, rng.randint(-2, 3), rng.randint(-2, 3)) for a in accounts]
        x = rng.random()
        if x < 0.15:
            row.pop(rng.randrange(len(row)))
        elif x < 0.25:
            row[rng.randrange(len(row))] = (row[0][0] + 1000, 1, 1)
        elif x < 0.35:
            k = rng.randrange(len(row))
            row[k] = (row[k][0], NIL)
        rng.shuffle(row)
        rows.append(row)
    return rows


def plant_forks(history, opts, n=1):
    """(history + n fork blocks, {"R": [...], "R2": [...]} the history indexes of the forked reads).  The ledger's transfers must all have
    completed :ok or :fail (concurrent_ledger(..., info=0, open_=0)): its final counters are then init + the :ok transfers."""
    accts = list(opts["accounts"])
    assert len(accts) >= 4
    cr = {a: opts["initial"][a]["credits-posted"] for a in accts}
    db = {a: opts["initial"][a]["debits-posted"] for a in accts}
    open_ = {}
    for op in history:
        if not isinstance(op.get("process"), int) or not op["value"] or op["value"][0][0] != "t":
            continue
        if op["type"] == "invoke":
            open_[op["process"]] = op
        else:
            assert op["type"] in ("ok", "fail") and op["process"] in open_, "plant_forks: a transfer that did not complete :ok or :fail"
            invoked = open_.pop(op["process"])
            for _t, _i, m in (invoked["value"] if op["type"] == "ok" else ()):
                cr[m["credit-acct"]] += m["amount"]; db[m["debit-acct"]] += m["amount"]
    assert not open_, "plant_forks: an open transfer"
    hist = list(history)
    planted = {"R": [], "R2": []}
    ident = 1 + max([m[1] for op in history if op["value"] and op["value"][0][0] == "t" for m in op["value"]] + [0])
    base = 1 + max([op["process"] for op in history if isinstance(op.get("process"), int)] + [0])
    snap = lambda c, d: [["r", a, {"credits-posted": c[a], "debits-posted": d[a]}] for a in accts]
    for k in range(n):
        a, b, c, d = (accts[(4 * k + j) % len(accts)] for j in range(4))
        t1 = [["t", ident, {"debit-acct": a, "credit-acct": b, "amount": 1 + k % 3}]]
        t2 = [["t", ident + 1, {"debit-acct": c, "credit-acct": d, "amount": 2}]]
        ident += 2
        p = base + 4 * k
        _op(hist, p, "invoke", t1); _op(hist, p + 1, "invoke", t2)
        _op(hist, p + 2, "invoke", [["r", x, None] for x in accts]); _op(hist, p + 3, "invoke", [["r", x, None] for x in accts])
        c1, d1 = dict(cr), dict(db)
        c1[b] += t1[0][2]["amount"]; d1[a] += t1[0][2]["amount"]
        c2, d2 = dict(cr), dict(db)
        c2[d] += 2; d2[c] += 2
        _op(hist, p + 2, "ok", snap(c1, d1)); planted["R"].append(len(hist) - 1)
        _op(hist, p + 3, "ok", snap(c2, d2)); planted["R2"].append(len(hist) - 1)
        _op(hist, p, "ok", t1); _op(hist, p + 1, "ok", t2)
        cr[b] += t1[0][2]["amount"]; db[a] += t1[0][2]["amount"]; cr[d] += 2; db[c] += 2
    return hist, planted


def forked_ledger(seed, forks=1, **kw):
    h, o, _ = G.concurrent_ledger(seed, info=0.0, open_=0.0, **kw)
    h2, planted = plant_forks(h, o, forks)
    return h2, o, planted


def _skewed(u, v):
    return any(u[k] < v[k] for k in u if k in v) and any(v[k] < u[k] for k in u if k in v)


def torn_ledger(seed, **kw):
    """(history, opts, the torn read's history index): a valid concurrent ledger in which one read takes half its accounts from a later read"""
    h, o, _ = G.concurrent_ledger(seed, **kw)
    accts = o["accounts"]
    rng = random.Random(seed)
    reads = [i for i, op in enumerate(h) if op["type"] == "ok" and op["value"] and op["value"][0][0] == "r"]
    vec = lambda value: {(a, f): m[f] for _r, a, m in value for f in FIELDS}
    bal = lambda value, half: sum(m["credits-posted"] - m["debits-posted"] for _r, a, m in value if a in half)
    for _ in range(200):
        half = set(rng.sample(accts, len(accts) // 2))
        for i, r in enumerate(reads):
            for s in reads[i + 2:]:
                if bal(h[r]["value"], half) != bal(h[s]["value"], half):
                    continue
                value = [m2 if m[1] in half else m for m, m2 in zip(h[r]["value"], h[s]["value"])]
                if any(_skewed(vec(value), vec(h[q]["value"])) for q in reads if q != r):
                    return h[:r] + [dict(h[r], value=value)] + h[r + 1:], o, r
    raise AssertionError("torn_ledger: no balanced half found")


# ---------------------------------------------------------------- shape cases: the smallest at which the kernels can go wrong

def chain_rows(accounts, n, pairs_at=(), rng=None, base=10):
    """n reads of every account in a chain (read k holds base + k on every counter), in a shuffled order, where the chain's members k and
    k + 1 for k in pairs_at are made incomparable (one skewed pair each, with nobody else)"""
    rows = []
    for k in range(n):
        row = [(a, base + k, base + k) for a in accounts]
        if k in pairs_at:
            row[-1] = (accounts[-1], base + k, base + k + 1)
        if k - 1 in pairs_at:
            row[-1] = (accounts[-1], base + k, base + k - 1)
        rows.append(row)
    if rng is not None:
        rng.shuffle(rows)
    return rows


def shape_cases(big=True):
    """[{"name", "history", "opts", "counts": {summary field (or "skewed"): value the case was built for}}]
    big: with the cases of more than 16,000 reads (the device's own chunk edges; the emulator reaches those paths by its plan's knobs)"""
    rng = random.Random(7)
    cases = []

    def add(name, hist_opts, **counts):
        h, o = hist_opts
        cases.append({"name": name, "history": h, "opts": o, "counts": counts})

    A1, A2, A8 = [7], [3, 1], list(range(1, 9))
    valid = dict(skewed=0, n_pairs=0, n_candidates=0, n_partial=0)
    # read and account counts
    add("no-reads", G.staged_ledger(A8, [[(1, 2, 3)]] * 4, n_reads=0), read_count=0, n_checked=0, **valid)
    add("one-read", reads_ledger(A2, chain_rows(A2, 1)), read_count=1, n_checked=2, **valid)
    add("two-equal-reads", reads_ledger(A2, [[(3, 5, 5), (1, 5, 5)]] * 2), read_count=2, n_checked=4, **valid)
    add("two-skewed-reads", reads_ledger(A2, [[(3, 5, 6), (1, 5, 5)], [(3, 6, 5), (1, 5, 5)]]), skewed=2, n_pairs=1, n_candidates=2)
    add("one-account", reads_ledger(A1, [[(7, 5, 1)], [(7, 4, 2)], [(7, 9, 9)]]), skewed=2, n_pairs=1, n_candidates=2, n_checked=3)
    add("eight-accounts-valid", G.staged_ledger(A8, [[(rng.choice(A8), rng.choice(A8), rng.randint(0, 9))] for _ in range(40)]), n_checked=24, **valid)
    A33 = list(range(100, 133))
    add("33-accounts", reads_ledger(A33, chain_rows(A33, 9, pairs_at=(4,), rng=rng), transfers_first=3), n_checked=9 * 33, skewed=2, n_pairs=1, n_candidates=2)
    A1025 = list(range(2050, 0, -2))                                            # (descending: a counter is the account's position in this list)
    add("1025-accounts", reads_ledger(A1025, chain_rows(A1025, 5, pairs_at=(1,), rng=rng)), n_checked=5 * 1025, skewed=2, n_pairs=1, n_candidates=2)
    add("1025-accounts-valid", reads_ledger(A1025, chain_rows(A1025, 3, rng=rng)), n_checked=3 * 1025, **valid)
    # edges of the sort, the scan and the tiles: 64 reads are a wavefront's step of the sort, a chunk of the scan and a tile of the pair
    # kernel; 256 candidates are a block of the pair kernel (an antichain: every read is one); past 16,384 reads a chunk of the sort is two
    # wavefronts' worth and the scan's carry over the chunks takes a second step of 256
    for n in (63, 64, 65, 127, 128, 129):
        add(f"chain-of-{n}", reads_ledger(A2, chain_rows(A2, n, pairs_at=(0, n - 2), rng=rng)), read_count=n, skewed=4, n_pairs=2, n_candidates=4, n_checked=2 * n)
        add(f"valid-chain-of-{n}", reads_ledger(A2, chain_rows(A2, n, rng=rng)), read_count=n, n_checked=2 * n, **valid)
    for n in (255, 256, 257):
        add(f"antichain-of-{n}", reads_ledger(A1, [[(7, k, n - 1 - k)] for k in range(n)]), read_count=n, skewed=n, n_pairs=n * (n - 1) // 2, n_candidates=n)
    if big:
        for n in (16383, 16384, 16385):
            add(f"chain-of-{n}", reads_ledger(A1, chain_rows(A1, n, pairs_at=(0, 8000, n - 2), rng=rng)), read_count=n, skewed=6, n_pairs=3, n_candidates=6, n_checked=n)
    # sums that differ only in their lowest byte, only in their highest, and in sign
    low = [[(7, k, 0)] for k in range(256)]
    rng.shuffle(low)
    add("sums-lowest-byte", reads_ledger(A1, low), read_count=256, **valid)
    high = [[(7, k << 56, k + 64)] for k in range(-63, 64)]
    rng.shuffle(high)
    add("sums-highest-byte-and-sign", reads_ledger(A1, high), read_count=127, **valid)
    mixed = [[(7, rng.choice((-1, 1)) * rng.randrange(2 ** 61), rng.randrange(100))] for _ in range(150)]
    add("sums-every-byte", reads_ledger(A1, mixed), read_count=150)
    add("equal-sums", reads_ledger(A2, [[(3, 1, 4), (1, 2, 3)], [(3, 4, 1), (1, 3, 2)], [(3, 1, 4), (1, 2, 3)], [(3, 2, 3), (1, 2, 3)]]), skewed=4, n_pairs=5, n_candidates=4)
    add("identical-reads", reads_ledger(A8, [[(a, 5 * a, a) for a in A8]] * 200), read_count=200, n_checked=1600, **valid)
    # skew patterns
    add("antichain-of-300", reads_ledger(A1, [[(7, k, 299 - k)] for k in range(300)]), skewed=300, n_pairs=44850, n_candidates=300)
    rows = chain_rows(A8, 100, rng=rng)
    rows.insert(50, [(a, 200, 200) for a in A8[:-1]] + [(8, 0, 0)])             # above everybody but on account 8, where it is below
    add("one-outlier", reads_ledger(A8, rows), read_count=101, skewed=101, n_pairs=100, n_candidates=101)
    # a complete read skewed ONLY with a partial one: it is no candidate, its count and its partner arrive by atomics
    rows = chain_rows(A2, 70, rng=rng, base=20) + [[(3, 5, 5), (1, 5, 5)], [(3, 6, 4)]]
    add("complete-skewed-with-partial-only", reads_ledger(A2, rows), read_count=72, skewed=2, n_pairs=1, n_candidates=1, n_partial=1)
    # partial and unchecked reads
    rows = chain_rows(A8, 20, rng=rng)
    rows[3] = rows[3][:-1]                                                      # lacks account 8
    rows[9] = rows[9][:2] + [(3, NIL)] + rows[9][3:]                            # account 3 nil
    rows[15] = rows[15][:5] + [(77, 1, 1)] + rows[15][6:]                       # a foreign id in account 6's place
    add("partial-reads", reads_ledger(A8, rows), n_partial=3, n_candidates=3, n_checked=157)
    rows = [[(3, k, 100 - k)] if k % 2 else [(1, k, k)] for k in range(90)]
    add("partial-reads-only", reads_ledger(A2, rows), n_partial=90, n_candidates=90, n_checked=90, skewed=45, n_pairs=45 * 44 // 2)
    ids = list(range(1, 301))
    rows = [[(i, (k if i in A8 else rng.randrange(1000)), k) for i in ids] for k in range(6)]
    add("long-reads-with-foreign-ids", reads_ledger(A8, rows), read_count=6, n_checked=48, **valid)
    # values
    add("negative-counters", reads_ledger(A2, [[(3, -5, -9), (1, -7, -7)], [(3, -6, -8), (1, -7, -7)], [(3, -9, -9), (1, -9, -9)]]), skewed=2, n_pairs=1)
    add("near-2^62", reads_ledger(A1, [[(7, 2 ** 62 - 1 - k, 2 ** 62 - k)] for k in range(5)] + [[(7, -(2 ** 62) + 3, 2 ** 62 + 1)]]), read_count=6, skewed=6, n_pairs=5)
    add("extremes-of-int64", reads_ledger(A2, [[(3, 2 ** 63 - 1, 0), (1, 0, 0)], [(3, 0, 0), (1, -(2 ** 63 - 1), 0)], [(3, 1, -1), (1, -1, 1)]]), read_count=3, skewed=3, n_pairs=2)
    # planted histories
    h, o, planted = forked_ledger(31, forks=2, workers=5, ops=220)
    add("planted-fork", (h, o), skewed=4, n_pairs=2, n_partial=0)
    h, o, _r = torn_ledger(32, workers=5, ops=220)
    add("planted-torn", (h, o), n_partial=0)
    for name in G.ANOMALIES:                                                   # the realtime plants substitute other true snapshots: no skew
        h, o, planted = G.concurrent_ledger(11, workers=5, ops=150, plant=(name,))
        assert name in planted
        add("realtime-planted-" + name, (h, o), **valid)
    return cases

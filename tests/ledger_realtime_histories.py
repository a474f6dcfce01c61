"""TEST INFRASTRUCTURE.  Seeded CONCURRENT ledger histories for the realtime checker (jepsen/ledger.py RealtimeBounds), and the shape
cases its emulator and GPU tests share.

`concurrent_ledger` simulates workers that hold ops open across each other: every op is invoked, takes effect at some later step and
completes at a still later one, the steps of all workers interleaved by the seed.  A transfer's outcome is drawn at its invocation: ok
(applies, completes :ok), fail (does not apply, completes :fail), info (applies or not, completes :info) or open (applies or not, never
completes: its worker goes on under a new process, as Jepsen's does).  Transfers carry one to three micro-ops, self-transfers and
amount 0 among them.  A read returns the counters as they are when it takes effect, so the history is valid by construction.

Planted anomalies, by name -- `planted[name]` is the history index of the read that carries it:
  stale      the read returns the initial snapshot although a transfer of a positive amount completed :ok before its invocation
  future     the read returns the final counters although one of them includes a transfer invoked after the read completed
  regressed  the read returns an earlier read's smaller counter after a read that saw a greater one had completed
"""
import random

ANOMALIES = ("stale", "future", "regressed")
FIELDS = ("credits-posted", "debits-posted")


def _snapshot(accounts, cr, db):
    return [["r", a, {"credits-posted": cr[a], "debits-posted": db[a]}] for a in accounts]


def concurrent_ledger(seed, workers=4, ops=60, accounts=8, read_share=0.45, fail=0.1, info=0.1, open_=0.05, max_mops=3, plant=(), funded=100):
    rng = random.Random(seed)
    accts = list(range(1, accounts + 1))
    init = {a: {"credits-posted": funded, "debits-posted": 0} for a in accts}
    cr, db = {a: funded for a in accts}, {a: 0 for a in accts}
    poss_cr, poss_db = dict(cr), dict(db)                      # what the transfers invoked so far that did not fail could add up to
    hist, w_state, next_id, started = [], [None] * workers, 1, 0
    process = list(range(workers))
    reads = []                                                  # {"inv", "ret", "hi": (poss_cr, poss_db) at its completion}
    ok_done = []                                                # (completion index, the transfer's micro-ops) of :ok transfers with an amount > 0

    def emit(p, typ, value):
        hist.append({"type": typ, "f": "txn", "value": value, "process": p, "index": len(hist), "time": 1000 * (len(hist) + 1)})
        return len(hist) - 1

    while started < ops or any(s is not None for s in w_state):
        w = rng.randrange(workers)
        s = w_state[w]
        if s is None:
            if started >= ops:
                continue
            started += 1
            if rng.random() < read_share:
                value = [["r", a, None] for a in accts]
                w_state[w] = {"kind": "r", "step": 0, "inv": emit(process[w], "invoke", value), "outcome": "ok" if rng.random() > 0.1 else "info"}
            else:
                mops = []
                for _ in range(rng.randint(1, max_mops)):
                    d = rng.choice(accts)
                    c = d if rng.random() < 0.1 else rng.choice(accts)
                    mops.append(["t", next_id, {"debit-acct": d, "credit-acct": c, "amount": rng.choice((0, 1, 1, 2, 3, 5))}])
                    next_id += 1
                x = rng.random()
                outcome = "fail" if x < fail else "info" if x < fail + info else "open" if x < fail + info + open_ else "ok"
                applies = outcome == "ok" or (outcome in ("info", "open") and rng.random() < 0.5)
                if outcome != "fail":
                    for _t, _i, m in mops:
                        poss_cr[m["credit-acct"]] += m["amount"]; poss_db[m["debit-acct"]] += m["amount"]
                w_state[w] = {"kind": "t", "step": 0, "inv": emit(process[w], "invoke", mops), "outcome": outcome, "applies": applies, "mops": mops}
        elif s["step"] == 0:                                    # the op takes effect
            s["step"] = 1
            if s["kind"] == "r":
                s["value"] = _snapshot(accts, cr, db)
            elif s["applies"]:
                for _t, _i, m in s["mops"]:
                    cr[m["credit-acct"]] += m["amount"]; db[m["debit-acct"]] += m["amount"]
        else:                                                   # the op completes
            w_state[w] = None
            if s["kind"] == "r":
                if s["outcome"] == "ok":
                    ret = emit(process[w], "ok", s["value"])
                    reads.append({"inv": s["inv"], "ret": ret, "hi": (dict(poss_cr), dict(poss_db))})
                else:
                    emit(process[w], "info", [["r", a, None] for a in accts])
                    process[w] += workers
            elif s["outcome"] == "open":
                process[w] += workers
            else:
                ret = emit(process[w], s["outcome"], s["mops"])
                if s["outcome"] == "info":
                    process[w] += workers
                if s["outcome"] == "ok" and any(m["amount"] > 0 for _t, _i, m in s["mops"]):
                    ok_done.append(ret)
    planted = {}
    value_of = lambda r: {a: m for _r, a, m in hist[r["ret"]]["value"]}
    taken = set()
    for name in plant:
        assert name in ANOMALIES, name
        if name == "stale":
            cands = [r for r in reads if ok_done and ok_done[0] < r["inv"] and r["ret"] not in taken]
            if cands:
                r = cands[len(cands) // 2]
                hist[r["ret"]] = dict(hist[r["ret"]], value=[["r", a, dict(init[a])] for a in accts])
                planted[name] = r["ret"]; taken.add(r["ret"])
        elif name == "future":
            final = (cr, db)
            for r in reads:
                if r["ret"] not in taken and any(final[x][a] > r["hi"][x][a] for x in (0, 1) for a in accts):
                    hist[r["ret"]] = dict(hist[r["ret"]], value=_snapshot(accts, cr, db))
                    planted[name] = r["ret"]; taken.add(r["ret"])
                    break
        else:
            done = False
            for i2 in range(len(reads) - 1, -1, -1):
                r2 = reads[i2]
                if r2["ret"] in taken:
                    continue
                for r1 in reads:
                    if not (r1["ret"] < r2["inv"]) or r1["ret"] in taken:
                        continue
                    for r0 in reads:
                        if r0["ret"] in taken or r0 is r1 or r0 is r2:
                            continue
                        v0, v1 = value_of(r0), value_of(r1)
                        if any(v0[a][f] < v1[a][f] for a in accts for f in FIELDS):
                            hist[r2["ret"]] = dict(hist[r2["ret"]], value=[["r", a, dict(v0[a])] for a in accts])
                            planted[name] = r2["ret"]; taken.add(r2["ret"]); done = True
                            break
                    if done:
                        break
                if done:
                    break
    opts = {"accounts": accts, "initial": init, "total-amount": funded * accounts, "negative-balances?": False}
    return hist, opts, planted


# ---------------------------------------------------------------- shape cases: the smallest at which the kernels can go wrong

def _op(hist, p, typ, value):
    hist.append({"type": typ, "f": "txn", "value": value, "process": p, "index": len(hist), "time": 1000 * (len(hist) + 1)})


def _t(ident, d, c, amount):
    return ["t", ident, {"debit-acct": d, "credit-acct": c, "amount": amount}]


def staged_ledger(accts, transfers, n_reads=3, reverse_completion=False, reads_without_invocation=False, read_ids=None, init=None):
    """`transfers` (lists of (debit, credit, amount) micro-ops) invoked one after the other by processes of their own, completed :ok in
    the same or the reverse order, with a read before, between and after; the reads return the true counters, so the history is valid."""
    init = init or {}
    cr = {a: init.get(a, {}).get("credits-posted", 0) for a in accts}
    db = {a: init.get(a, {}).get("debits-posted", 0) for a in accts}
    read_ids = list(accts) if read_ids is None else read_ids
    hist, ident = [], 1

    def read(p):
        if not reads_without_invocation:
            _op(hist, p, "invoke", [["r", a, None] for a in read_ids])
        _op(hist, p, "ok", [["r", a, {"credits-posted": cr.get(a, 0), "debits-posted": db.get(a, 0)}] for a in read_ids])

    if n_reads:
        read(0)
    values = []
    for k, mops in enumerate(transfers):
        v = []
        for d, c, amount in mops:
            v.append(_t(ident, d, c, amount)); ident += 1
        values.append(v)
        _op(hist, 10 + k, "invoke", v)
    order = range(len(transfers) - 1, -1, -1) if reverse_completion else range(len(transfers))
    for n, k in enumerate(order):
        for _t0, _i, m in values[k]:
            if m["credit-acct"] in cr: cr[m["credit-acct"]] += m["amount"]
            if m["debit-acct"] in db: db[m["debit-acct"]] += m["amount"]
        _op(hist, 10 + k, "ok", values[k])
        if n_reads > 2 and n == len(transfers) // 2:
            read(1)
    if n_reads > 1:
        read(2)
    return hist, {"accounts": list(accts), "initial": init}


def shape_cases():
    """[{"name", "history", "opts", "counts": {summary field or "reads" / "read_mops": value the case was built for}}]"""
    rng = random.Random(5)
    cases = []

    def add(name, hist_opts, **counts):
        h, o = hist_opts
        cases.append({"name": name, "history": h, "opts": o, "counts": counts})

    A8 = list(range(1, 9))
    few = lambda n, accts: [[(rng.choice(accts), rng.choice(accts), rng.randint(0, 9))] for _ in range(n)]
    add("no-reads", staged_ledger(A8, few(5, A8), n_reads=0), read_count=0, n_possible=5)
    add("no-transfers", staged_ledger(A8, [], n_reads=2), read_count=2, n_possible=0, n_definite=0, n_checked=16)
    add("one-account", staged_ledger([7], few(9, [7])), n_checked=3, n_possible=9)
    add("eight-accounts", staged_ledger(A8, few(40, A8)), n_checked=24, n_definite=40)
    A65 = list(range(100, 165))
    add("65-accounts", staged_ledger(A65, few(90, A65)), n_checked=195)
    A1025 = list(range(1, 2051, 2))
    add("1025-accounts", staged_ledger(A1025, few(70, A1025), n_reads=2), n_checked=2050)
    # one account's list of length 0, 1, 63, 64, 65 (and the chunk is 64 entries: chunk +- 1); account 1 is credited n times, 2 debited
    for n in (0, 1, 63, 64, 65):
        add(f"list-of-{n}", staged_ledger([1, 2, 3], [[(2, 1, 1)]] * n + [[(3, 3, 2)]] * 3), n_possible=n + 3)
    # a stream of one chunk -+ one micro-op: 62, 64, 66 entries (two per micro-op) of 64 a chunk
    for n in (31, 32, 33):
        add(f"chunk-of-{2 * n}-entries", staged_ledger(A8, few(n, A8)), n_possible=n, n_definite=n)
    # a transfer of five micro-ops straddling the chunk edge (entries 60 .. 69 of 2 per micro-op)
    add("straddle", staged_ledger(A8, few(30, A8) + [[(1, 2, 3), (2, 3, 4), (3, 1, 5), (1, 1, 6), (4, 2, 7)]] + few(10, A8)), n_possible=41)
    add("all-on-one-account", staged_ledger([4], [[(4, 4, k % 7)] for k in range(150)]), n_possible=150, foreign_sides=0)
    add("reverse-completion", staged_ledger(A8, few(70, A8), reverse_completion=True), n_definite=70)
    long_ids = list(range(1, 301))
    add("long-read", staged_ledger(long_ids, few(20, long_ids[:10]), n_reads=2), read_count=2, n_checked=600)
    add("reads-without-invocation", staged_ledger(A8, few(12, A8), reads_without_invocation=True), read_count=3)
    add("foreign-and-unchecked", staged_ledger(A8, [[(1, 99, 3)], [(98, 2, 4)], [(3, 4, 5)]], read_ids=[1, 2, 77, 3]), foreign_sides=2, n_checked=9)
    # a miss that saturates: the least counter the columns hold, -(2^63 - 1), under a lower bound of 5
    h, o = staged_ledger([1, 2], [[(1, 2, 5)]], n_reads=2)
    h[-1] = dict(h[-1], value=[["r", 2, {"credits-posted": -(2 ** 63 - 1), "debits-posted": 0}]])
    add("saturated-miss", (h, o), error_count=1)
    for name in ANOMALIES:                                     # every kind of violation through the finish and the summary
        h, o, planted = concurrent_ledger(11, workers=5, ops=150, plant=(name,))
        assert name in planted
        add("planted-" + name, (h, o))
    h, o, planted = concurrent_ledger(12, workers=6, ops=200, plant=ANOMALIES)
    add("planted-all", (h, o))
    return cases

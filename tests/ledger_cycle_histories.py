"""TEST INFRASTRUCTURE.  Histories for the cycle search over the ledger's reads (jepsen/ledger.py "Cycle search"): the curated cases its
host, emulator and GPU tests share, and a seeded random generator.

`timed_reads` makes a history of reads alone from rows and explicit slots in time: a read is (row, inv, ret) -- row a list of
(id, credits, debits) or (id, NIL), inv / ret the slots of its invocation and its :ok completion, inv None for a read that has no
invocation.  Every read has a process of its own, so pairing is trivial; reads are numbered in the order of ret."""
import random

import ledger_snapshot_histories as S

NIL = S.NIL


def timed_reads(accounts, reads):
    events = []
    for k, (row, inv, ret) in enumerate(reads):
        assert inv is None or inv < ret
        if inv is not None:
            events.append((inv, 0, k))
        events.append((ret, 1, k))
    events.sort()
    assert len({e[0] for e in events}) == len(events), "two events in one slot"
    hist = []
    for _slot, done, k in events:
        row = reads[k][0]
        value = [["r", m[0], None if (not done or m[1] is NIL) else {"credits-posted": m[1], "debits-posted": m[2]}] for m in row]
        hist.append({"type": "ok" if done else "invoke", "f": "txn", "value": value, "process": k, "index": len(hist), "time": 1000 * (len(hist) + 1)})
    return hist, {"accounts": list(accounts)}


def concurrent(accounts, rows):
    """every read invoked before any completes: no realtime edge; read k is rows[k]"""
    n = len(rows)
    return timed_reads(accounts, [(row, k, n + k) for k, row in enumerate(rows)])


def full(accounts, v):
    return [(a, v, v) for a in accounts]


def core_path(m, closed, n_clean=0, shift=0):
    """m partial reads P_0 -> P_1 -> ... -> P_(m-1), each edge monotonic on an account only its two ends check, closed into one cycle by
    P_(m-1) -> P_0 or left open; n_clean complete reads above them all (every P has an edge to them, none comes back), all concurrent.
    (accounts, rows)"""
    accounts = list(range(10 + shift, 10 + shift + m + 1))
    rows = []
    for i in range(m):
        nxt = accounts[(i + 1) % m] if closed else accounts[i + 1]
        rows.append([(accounts[i], 2, 2)] + ([(nxt, 1, 1)] if nxt != accounts[i] else []))
    rows += [full(accounts, 5 + k) for k in range(n_clean)]
    return accounts, rows


def cases():
    """[{"name", "history", "opts", "counts": {summary field: the value the case was built for}}]"""
    out = []

    def add(name, hist_opts, **counts):
        h, o = hist_opts
        out.append({"name": name, "history": h, "opts": o, "counts": counts})

    A2, A3 = [1, 2], [1, 2, 3]
    # a 3-cycle through three partial reads: no skewed pair, no regressed read
    add("three-partial-cycle", concurrent(A3, [[(1, 5, 5), (2, 1, 1)], [(2, 2, 2), (3, 1, 1)], [(3, 2, 2), (1, 4, 4)]]),
        n_partial=3, n_core=3, n_on_cycle=3, n_components=1, first=0, largest=0, largest_size=3)
    # P -> C ~> C' -> P through clean reads only: P is below C, C' returned before P was invoked
    add("through-clean-reads", timed_reads(A2, [(full(A2, 1), 0, 1), (full(A2, 2), 2, 3), ([(1, 0, 0)], 4, 5)]),
        n_core=1, n_on_cycle=3, n_components=1, largest_size=3)
    add("through-clean-reads-monotonic", concurrent(A3, [full(A3, 1), full(A3, 2), [(1, 0, 0), (2, 3, 3)]]), n_core=1, n_on_cycle=3)
    # the equal-class cases: s_out(P) == s_in(P'), one class of clean reads (5 everywhere); the return edge P' -> P is monotonic on a
    # counter where no clean read is below P.  C2 has C's vector and lies outside by the realtime tie on the component's hi class.
    #   monotonic out, realtime in: P below C; C returned before P' was invoked; P spans everything
    add("equal-class-monotonic-out", timed_reads(A2, [([(1, 4, 4)], 0, 20), (full(A2, 5), 1, 2), ([(1, 3, 3)], 5, 6), (full(A2, 5), 4, 7)]),
        n_core=2, n_on_cycle=3, n_components=1, largest_size=3)
    #   realtime out, monotonic in: P returned before C was invoked; C below P' on account 1; P' spans everything
    add("equal-class-monotonic-in", timed_reads(A3, [([(1, 6, 6), (2, 3, 3)], 0, 20), ([(2, 5, 5)], 1, 3), (full(A3, 5), 4, 5)]),
        n_core=2, n_on_cycle=3, n_components=1, largest_size=3)
    #   the lo class by realtime alone: P' -> P -> C in real time, C below P'.  C0 has C's vector and lies outside by the realtime tie on
    #   the component's lo class (it was invoked before anybody returned)
    add("lo-class-realtime-tie", timed_reads(A2, [([(1, 6, 6)], 1, 2), ([(2, 5, 5)], 3, 4), (full(A2, 5), 5, 6), (full(A2, 5), 0, 7)]),
        read_count=4, n_core=2, n_on_cycle=3, n_components=1, largest_size=3)
    add("equal-class-both-monotonic", concurrent(A3, [[(2, 4, 4)], full(A3, 5), [(1, 6, 6), (2, 3, 3)]]), n_core=2, n_on_cycle=3, n_components=1)
    #   realtime on both sides: P -> C -> P' in real time is a direct edge P -> P' and no more
    add("equal-class-realtime-both", timed_reads(A3, [([(2, 5, 5)], 0, 1), (full(A3, 5), 2, 3), ([(2, 3, 3)], 4, 5)]), n_core=2, n_on_cycle=3, n_components=1)
    add("equal-class-realtime-both-open", timed_reads(A3, [([(2, 5, 5)], 0, 1), (full(A3, 5), 2, 3), ([(2, 5, 5)], 4, 5)]), n_core=2, n_on_cycle=0)
    # sizes: the reads' and the core's word edges
    for n in (63, 64, 65):
        add(f"{n}-reads-cycle-of-5", concurrent(*core_path(5, True, n - 5)), read_count=n, n_core=5, n_on_cycle=5, n_components=1)
    add("core-of-0", concurrent(A2, [full(A2, k) for k in range(40)]), n_core=0, n_on_cycle=0, closure_rounds=0, valid=1)
    for m in (1, 31, 32, 33, 63, 64, 65):
        add(f"core-cycle-of-{m}", concurrent(*core_path(m, True, 3)), n_core=m, n_on_cycle=m if m > 1 else 0, n_components=int(m > 1))
    add("core-path-of-70-closed", concurrent(*core_path(70, True, 2)), n_core=70, n_on_cycle=70, n_components=1, largest_size=70)
    add("core-path-of-70-open", concurrent(*core_path(70, False, 2)), n_core=70, n_on_cycle=0, valid=1)
    a1, r1 = core_path(4, True)
    a2, r2 = core_path(7, True, shift=50)
    add("two-components", concurrent(a1 + a2, r2[:3] + r1 + r2[3:]), n_core=11, n_on_cycle=11, n_components=2, first=0, largest=0, largest_size=7)
    # all complete
    add("all-complete-valid", S.reads_ledger(A2, S.chain_rows(A2, 100)), n_core=0, n_on_cycle=0, closure_rounds=0, valid=1)
    h, o, _planted = S.forked_ledger(31, forks=1, workers=5, ops=120)
    add("all-complete-long-fork", (h, o), n_partial=0, n_components=1)
    h, o, planted = S.G.concurrent_ledger(11, workers=5, ops=150, plant=("regressed",))
    add("all-complete-regressed", (h, o), n_partial=0)
    # reads without an invocation, a read that checks nothing, negative counters, equal sums with unequal partial vectors
    add("no-invocation", timed_reads(A2, [(full(A2, 2), None, 1), ([(1, 1, 1)], None, 2), (full(A2, 1), 3, 4), ([(2, 0, 0)], None, 5)]), n_partial=2)
    add("checks-nothing", timed_reads(A2, [([(77, 1, 1)], 0, 1), (full(A2, 2), 2, 3), ([(1, NIL), (2, NIL)], 4, 5), (full(A2, 1), 6, 7)]), n_partial=2)
    add("negative-counters", concurrent(A3, [[(1, -5, -5), (2, -9, -9)], [(2, -8, -8), (3, -9, -9)], [(3, -8, -8), (1, -6, -6)], full(A3, -7)]), n_on_cycle=4)
    add("equal-sums-unequal-partials", concurrent(A3, [[(1, 1, 4), (2, 2, 3)], [(1, 4, 1), (2, 3, 2)], [(2, 1, 4), (3, 5, 0)], full(A3, 2), full(A3, 2)]), n_partial=3)
    return out


def random_history(rng):
    """1-4 accounts, up to 12 reads in a random interleaving: some partial, some without an invocation, some that check nothing, few
    distinct values (equal sums) and negative counters"""
    accounts = rng.sample(range(1, 9), rng.randint(1, 4))
    n = rng.randint(1, 12)
    monotone = rng.random() < 0.5                     # (half the histories: mostly growing counters, so that many reads stay clean)
    slots = list(range(2 * n))
    rng.shuffle(slots)
    reads = []
    for k in range(n):
        base = k // 2 if monotone else 0
        row = [(a, base + rng.randint(-2, 1), base + rng.randint(-1, 1)) if not monotone or rng.random() < 0.3 else (a, base, base) for a in accounts]
        x = rng.random()
        if x < 0.2:
            row = rng.sample(row, rng.randint(1, len(row) - 1)) if len(row) > 1 else [(99, 1, 1)]
        elif x < 0.27:
            row[rng.randrange(len(row))] = (99, 1, 1)
        elif x < 0.34:
            j = rng.randrange(len(row))
            row[j] = (row[j][0], NIL)
        elif x < 0.38:
            row = [(99, 1, 1), (98, NIL)]
        a, b = sorted((slots[2 * k], slots[2 * k + 1]))
        reads.append((row, None if rng.random() < 0.12 else a, b))
    if monotone:                                      # (a growing ledger: the later a read returns the more it has seen)
        order = sorted(range(n), key=lambda k: reads[k][2])
        rows = [reads[k][0] for k in range(n)]
        for rank, k in enumerate(order):
            reads[k] = (rows[order[rank]] if rng.random() < 0.15 else [(m[0], m[1] + rank // 3, m[2] + rank // 3) if m[1] is not NIL else m for m in rows[k]], reads[k][1], reads[k][2])
    return timed_reads(accounts, reads)

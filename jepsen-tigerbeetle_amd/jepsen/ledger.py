"""tigerbeetle.tests.ledger -- the ledger workload's checkers (the reference's tests/ledger.clj:89-282, composed at :363-367).

Two statements of the same checkers:

* the HOST statement, plain Python written for clarity: `ledger_to_bank`, `BankChecker` (:SI), `UnexpectedOps`,
  `LookupAllInvokedTransfers`, `FinalReads`.  It is the specification the device route is tested against.
* the DEVICE route: `LedgerColumns` flattens the client ops into the columns of tbc_ledger_in (include/tbcheck.h), `check_columns`
  hands them to tbc_ledger_check (csrc/ledger_*.h) and builds the same three result maps from the arrays that come back.
  `unexpected-ops` returns ops and is O(ops): it stays on the host.

`test()` gives the workload's map with the composed checker; with `device_route=True` its SI, lookup-transfers and final-reads members
answer from ONE `check_columns` call.  :plot is not built.

Realtime bounds (`realtime_host` the specification, `realtime_numpy` the same in O(n log n), `RealtimeBounds` the checker,
`check_realtime_native` / `realtime_result_map` the device route over tbc_ledger_realtime; `test(realtime=True)` composes the member
"realtime").  Not in the reference: its :SI passes a read that is consistent but stale, one that shows a transfer nobody has invoked
yet, and two reads that go backwards in time.  credits-posted and debits-posted of an account only grow, so real time bounds every
counter a read returns -- a NECESSARY condition for strict serializability ("Ledger, Assumed Strict Serializable", the reference's
doc/LASS.md: its "compare w r" and "compare r r'" rules).  THE RULES, stated once here:

  Positions are indexes into the history.  Only client ops count (knossos.history.client_op); pairing is knossos.history.pair_index.
  A TRANSFER is a client invocation whose op_txn_f is "t": its micro-ops are the invocation's; inv(T) its index; its status the type
    of its completion (ok / fail / info, any other type reads as info), open if it has none; ret(T) the completion's index.  A transfer
    completion without an invocation is ignored.
  A READ is an :ok completion whose op_txn_f is "r" (the rows LedgerColumns.read_ops numbers): ret(R) its index, inv(R) its
    invocation's index, -1 if it has none (such a read gets no lower bound beyond the initial value).  Its micro-ops are the columns'
    ones: after ledger->bank's last-wins, nil maps flagged.  A micro-op that is nil, or whose id is no account, is NOT CHECKED (:SI
    reports those).
  BOUNDS of a checked micro-op of account a, per field x -- credits-posted: the transfer micro-ops with credit-acct = a;
    debits-posted: those with debit-acct = a; a self-transfer counts on both:
      lo    = init_x[a] + the amounts of the micro-ops of transfers with status ok and ret(T) < inv(R); 0 of them when the option
              "ok-transfers-apply?" is false (default true: what the Bank model assumes)
      hi    = init_x[a] + the amounts of the micro-ops of transfers with status /= fail and inv(T) < ret(R)
      floor = the greatest value of field x of account a over the reads R' with ret(R') < inv(R) that checked a; INT64_MIN if none
    A transfer micro-op that is nil, or a side of one that names no account, is skipped (the summary counts such sides, over the
    transfers that did not fail: `foreign_sides`, a nil micro-op counting as two).
  VIOLATIONS have a miss m > 0: stale m = lo - v, future m = v - hi, regressed m = floor - v.  A read's BITS: 1 stale credits,
    2 stale debits, 4 future credits, 8 future debits, 16 regressed credits, 32 regressed debits.  Its MISS per kind is the greatest
    over its micro-ops and both fields, 0 if none; misses saturate at INT64_MAX.
  SUMMARY: per kind count, first, last, worst as read numbers (worst: the greatest miss; ties go to the earliest read, as in
    tbc_ledger_errors); error_count = the reads with any bit, first_error the first of them, valid = none; n_definite = the
    transfers with status ok, n_possible = those that did not fail; n_checked = the read micro-ops checked.
  RANGES, so that no sum can wrap: every amount of a transfer that did not fail in [0, 2^31); fewer than 2^31 transfer micro-ops;
    |init| < 2^61.  ValueError here; tbc_ledger_realtime counts offending amounts on the device and answers TBC_ERR_UNSUPPORTED.
  OPTIONS: "accounts"; "initial" {account: {"credits-posted": c, "debits-posted": d}}, 0 where an account is not named (the test
    generators fund accounts with credits: they need it); "ok-transfers-apply?".

Snapshot order (`snapshots_host` the specification, `snapshots_numpy` the sort-and-scan statement the device is compared with,
`SnapshotOrder` the checker, `check_snapshots_native` / `snapshots_result_map` the device route over tbc_ledger_snapshots;
`test(snapshots=True)` composes the member "snapshots").  Not in the reference either: every checker above looks at one read at a time
(its total) or one counter at a time (its bounds in real time); none compares two reads ACROSS accounts, so a long fork -- R sees
transfer T1 and not T2, R' sees T2 and not T1, both concurrent -- passes them all.  The posted counters only grow and the workload's
reads read every account, so under serializability the reads of a history are a CHAIN under component-wise <=.  This is LASS.md's
discrete anomaly ("r and r' claim to have read some values in common, and in addition, each has read unique values") and the 2-cycle of
monotonic-key-graph in the reference's unfinished elle/core.clj.  THE RULES, stated once here:

  READS, their numbering and their micro-ops are those of the realtime rules: a read is an :ok completion whose op_txn_f is "r", a row
    of LedgerColumns.read_ops; its micro-ops are taken after ledger->bank's last-wins; a micro-op that is nil, or whose id is no
    account, is NOT CHECKED.
  A COUNTER is c = 2 k + x: k the account's position in `accounts`, x = 0 for credits-posted and 1 for debits-posted.  A read's VECTOR
    has a value at the counters it checks.  A read is COMPLETE if it checks every account, PARTIAL otherwise.
  R is BELOW R' on c if both check c and v_R[c] < v_R'[c].  R and R' (R /= R') are SKEWED if R is below R' on some c and R' is below R
    on some d.
  PER READ: skew_count the number of reads it is skewed with; skew_first the least read number among them, NO_OP if none; skew_key[2],
    against that first partner, the least counter on which the read is below it and the least on which it is above it (both NO_OP
    without a partner: MonotonicKeyExplainer's key, twice); snap_flags bit 1 partial, bit 2 skewed.
  SUMMARY: read_count, n_partial; n_checked = the read micro-ops checked; over the skewed reads count, first, last, worst (the greatest
    skew_count; ties go to the earliest read, as everywhere here); n_pairs = the unordered skewed pairs; valid = no read is skewed;
    n_candidates = n_partial + the complete reads skewed with a complete read (what the device's filter hands to its pair kernel).
  EXACT: with every read complete, "no two reads skewed" plus "no read regressed" (the realtime rules' bit) holds exactly when the
    graph of monotonic-key edges plus realtime edges over the reads is acyclic -- no SCC pass is needed.  The result map carries
    "exact?" = n_partial == 0.  With partial reads the rule is still SOUND (every skewed pair is an anomaly) but no longer the whole
    cycle search: a 3-cycle through partial reads needs no 2-cycle.
  RANGES: per read the sum of |v| over its checked counters < 2^63 (what LedgerColumns already refuses to exceed); negative counters are
    legal.  ValueError here; tbc_ledger_snapshots counts offending reads on the device and answers TBC_ERR_UNSUPPORTED.
  OPTIONS: "accounts".

Cycle search (`cycles_host` the specification -- the explicit graph and Tarjan --, `cycles_numpy` the reduction the device computes,
`CycleSearch` the checker, `check_cycles_native` / `cycles_result_map` the device route over tbc_ledger_cycles; `test(cycles=True)`
composes the member "cycles").  The snapshot rule is the whole cycle search only while every read is complete; a read that comes back
short is what a fault produces, and a cycle through partial reads needs no skewed pair and no regressed read.  This member decides
the graph the reference's unfinished elle/core.clj and doc/LASS.md ask for, partial reads included.  THE RULES, stated once here:

  READS, their numbering, their checked micro-ops, the COUNTERS c = 2 k + x and COMPLETE / PARTIAL are those of the snapshot rules;
    inv(R) and ret(R) those of the realtime rules, inv = -1 when a read has no invocation.
  EDGES over the reads.  MONOTONIC R -> R' on c: both check c and v_R[c] < v_R'[c].  REALTIME R -> R': ret(R) < inv(R'); a read with
    inv = -1 has no incoming realtime edge.  (The reachability of monotonic-key-graph united with Elle's realtime graph.)
  PER READ: scc[r] the least read number of r's strongly connected component when that component has two or more reads, NO_OP
    otherwise; cyc_flags[r] bit 1 partial, bit 2 on a cycle, bit 4 core.
  CORE.  U: the complete reads skewed with no complete read (each is comparable with every complete read).  C' in U is RT-FLAGGED if
    some C in U has ret(C) < inv(C') and sum(C) > sum(C') (sum: over all counters).  CLEAN = U minus the rt-flagged; CORE = every other
    read: partial, skewed with a complete read, or rt-flagged.  The clean reads alone are acyclic: every cycle passes through the core.
  SUMMARY: read_count, n_partial, n_core; n_on_cycle, n_components; first = the least read on a cycle; largest = the label of the
    largest component and largest_size its size (ties go to the earliest, as everywhere here); valid = (n_on_cycle == 0);
    closure_rounds = the boolean squarings of the core's m x m matrix A <- A | A.A, the one that changes nothing included (0 when the
    core is empty); n_checked = the read micro-ops checked; bad_values as in the snapshot rules.
  RANGES: those of the snapshot rules.  The device takes a core of at most 16,384 reads (TBC_LEDGER_CYCLES_MAX_CORE); above it
    tbc_ledger_cycles answers TBC_ERR_UNSUPPORTED with n_core filled, and the member answers "valid?" "unknown".
  OPTIONS: "accounts".

Journal audit (`journal_host` the specification, `journal_numpy` the vectorised statement the device is compared with, `JournalAudit`
the checker, `check_journal_native` / `journal_result_map` the device route over tbc_ledger_journal; `test(journal=True)` composes the
member "journal").  Not in the reference: an :ok :l-t lookup returns the ledger's JOURNAL -- every transfer's id, debit-acct, credit-acct
and amount -- and lookup-transfers asks one thing of it, and only of the final lookups: does it hold every invoked id.  A bit flipped
in an amount in every final lookup alike, a failed transfer journalled, an acknowledged transfer missing from a lookup, and balances
that hold a transfer twice (a duplicated packet keeps :SI's total, stays a chain, and hides under the slack :info transfers leave in
realtime's hi) pass every member above.  THE RULES, stated once here:

  Positions, client ops, pairing by process, a TRANSFER (its inv, ret and status), a READ (numbering, checked micro-ops, inv, ret), a
    COUNTER c = 2 k + x and init are those of the realtime and snapshot rules.
  RECORDS.  The micro-ops of the transfers (client invocations of kind "t"), in column order, are numbered 0 .. M-1.  The RECORD of an id
    is the first of them with that id; its OWNER is that micro-op's transfer.  A later micro-op with the same id is REINVOKED: counted
    in the summary, not a record.  A record may be nil.
  LOOKUPS.  A lookup is every :ok completion whose op_txn_f is "l-t", final or not, numbered in history order (tbc_ledger_check numbers
    only the final ones).  ret(L) is its index, inv(L) its invocation's index, -1 if it has none: nothing is before such a lookup.  Its
    micro-ops are its ENTRIES.
  PER ENTRY, entry_bits: 1 UNKNOWN its id has no record; 2 ALTERED its id has a record and the entry or the record is nil, or
    (debit-acct, credit-acct, amount) differ.  Both are judged entry by entry, so neither depends on order.
  PER LOOKUP AND RECORD.  A record is PRESENT in L if some entry of L has its id; present[L] the number of records present; REPEATED the
    entries with a record minus present[L].  A present record is FAILED if its owner's status is fail, EARLY if inv(owner) > ret(L).
    An absent record is LOST if its owner's status is ok, ret(owner) < inv(L) and "ok-transfers-apply?" holds (default true, as in
    realtime); VANISHED if some lookup L' with ret(L') < inv(L) has it present: the journal only grows.
  BOOKS.  J_L[c] = init[c] + the RECORD's amount for every record present in L that is not nil, on counter 2 k for its credit-acct and on
    2 k' + 1 for its debit-acct.  A side that names no account is skipped.  Altered and unknown entries are reported above and do not
    move the vector.  `foreign_sides` counts, over the records, the sides that name no account, a nil record counting as two.
  READS AGAINST BOOKS.  For a read R, a lookup L and a counter c that R checks: ret(R) < inv(L) and v_R[c] > J_L[c]: R is AHEAD of L (it
    saw money a later journal does not explain); ret(L) < inv(R) and v_R[c] < J_L[c]: R is BEHIND L.  Per lookup the number of reads
    ahead of it and behind it; per read rd_bits (1 ahead of some lookup, 2 behind some lookup) and rd_first[2], the least lookup number
    of each, NO_OP if none.
  KINDS: unknown, altered, repeated (entries), failed, early, lost, vanished (records), ahead, behind (reads): lk_counts[L][9].  Per
    transfer micro-op xfer_present, xfer_early, xfer_lost, xfer_vanished: numbers of lookups, 0 for a reinvoked micro-op; xfer_flags
    bit 1 reinvoked, bit 2 nil.
  SUMMARY: n_lookups, n_entries, n_xfer_mops, n_records, n_reinvoked, foreign_sides, bad_amounts, read_count, n_checked (the read
    micro-ops checked); per kind count, first, last, worst over the LOOKUPS with a non-zero count (worst: the greatest count; ties go
    to the earliest, as everywhere here) and the total; valid = every total is 0.
  CROSS-CHECK: for a :final? lookup, n_records - present[L] is lookup_missing of tbc_ledger_check.
  RANGES: every amount of a non-nil record in [0, 2^31); M < 2^31; fewer than 2^31 entries a lookup; |init| < 2^61.  ValueError here;
    tbc_ledger_journal counts offending amounts on the device and answers TBC_ERR_UNSUPPORTED.
  OPTIONS: those of realtime.

History ops are the dicts `edn.read_history` gives: "type" "f" "value" "process" "index" "time" "final?", keywords as strings; a
:value is a vector of micro-ops [f id m] with f in "t" "r" "l-t".

Where this departs from the reference, on purpose:
* err-badness of a wrong total is |total - total-amount|, an integer: the reference's (float (/ (- total expected) expected)) throws with
  its own default :total-amount 0 and collapses near values to equal floats.  The integer distance picks the same worst op wherever
  that float is defined and distinct.
* a read micro-op whose third element is nil has a nil balance (the reference's (- nil nil) throws); a client op whose :value is empty
  or nil has no first micro-op: ledger->bank drops it (the reference's `case` has no clause for it) and no checker counts it.
* `unequal-final-reads` / `unequal-final-lookups` are lists of the distinct values in order of first appearance (a Clojure set of
  vectors has no Python form).
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from .. import _native as N
from ..knossos import history as H
from ..knossos import model as M
from . import checker as jc
from .edn import _hashable

ERROR_TYPES = (None, "unexpected-key", "nil-balance", "wrong-total", "negative-value")       # by TBC_LEDGER_E_*
_KIND = {"t": N.LEDGER_K_TRANSFER, "r": N.LEDGER_K_READ, "l-t": N.LEDGER_K_LOOKUP}
_TYPE = {"invoke": N.LEDGER_T_INVOKE, "ok": N.LEDGER_T_OK, "fail": N.LEDGER_T_FAIL, "info": N.LEDGER_T_INFO}
_I64 = (-(2 ** 63), 2 ** 63)


def op_txn_f(op):
    """op->txn-f: the f of the op's first micro-op, None if its value is empty or nil."""
    v = op.get("value")
    return v[0][0] if v else None


# ---------------------------------------------------------------- the host statement

def _balance(m):
    return None if m is None else m["credits-posted"] - m["debits-posted"]


def _bank_op(op):
    """One client op under ledger->bank; None where it is dropped."""
    f = op_txn_f(op)
    if f == "r":
        if op["type"] == "ok":
            value = {}
            for _r, ident, m in op["value"]:
                value[ident] = _balance(m)
            return dict(op, f="read", value=value)
        return dict(op, f="read")
    if f == "t":
        return dict(op, f="transfer")
    return None


def ledger_to_bank(history):
    """ledger->bank (tests/ledger.clj:89-114).  Every op with a non-integer process is kept as it is."""
    out = []
    for op in history:
        if not H.client_op(op):
            out.append(op)
            continue
        b = _bank_op(op)
        if b is not None:
            out.append(b)
    return out


def err_badness(total_amount, err):
    t = err["type"]
    if t == "unexpected-key":
        return len(err["unexpected"])
    if t == "nil-balance":
        return len(err["nils"])
    if t == "wrong-total":
        return abs(err["total"] - total_amount)
    return -sum(err["negative"])


def check_op(accts, total, negative_balances, op):
    """check-op: the first error of an :ok read (a bank op), None if it has none."""
    value = op["value"]
    if any(k not in accts for k in value):
        return {"type": "unexpected-key", "unexpected": [k for k in value if k not in accts], "op": op}
    if any(b is None for b in value.values()):
        return {"type": "nil-balance", "nils": {k: b for k, b in value.items() if b is None}, "op": op}
    s = sum(value.values())
    if s != total:
        return {"type": "wrong-total", "total": s, "op": op}
    if not negative_balances and any(b < 0 for b in value.values()):
        return {"type": "negative-value", "negative": [b for b in value.values() if b < 0], "op": op}
    return None


def _max_by(f, xs):
    """jepsen.util/max-by: only a strictly greater element replaces the held one (ties: the earliest)."""
    best = None
    for x in xs:
        if best is None or f(x) > f(best):
            best = x
    return best


def _min_by(f, xs):
    best = None
    for x in xs:
        if best is None or f(x) < f(best):
            best = x
    return best


def _si_opts(test, opts):
    t = dict(opts or {})
    t.update(test or {})
    return (list(t.get("accounts") or range(1, 9)), t.get("total-amount") or 0, bool((opts or {}).get("negative-balances?", False)))


def _si_map(total_amount, read_count, groups):
    """the :SI result from {type: [error maps in history order]}"""
    errors = {}
    for t, errs in groups.items():
        e = {"count": len(errs), "first": errs[0], "worst": _max_by(lambda x: err_badness(total_amount, x), errs), "last": errs[-1]}
        if t == "wrong-total":
            e["lowest"] = _min_by(lambda x: x["total"], errs)
            e["highest"] = _max_by(lambda x: x["total"], errs)
        errors[t] = e
    firsts = [errs[0] for errs in groups.values()]
    return {"valid?": not groups, "read-count": read_count, "error-count": sum(len(e) for e in groups.values()),
            "first-error": _min_by(lambda x: x["op"]["index"], firsts), "errors": errors}


def _indexed(history):
    """the history with an "index" on every op (its position where it has none)"""
    return [op if "index" in op else dict(op, index=i) for i, op in enumerate(history)]


class BankChecker(jc.Checker):
    """:SI (tests/ledger.clj:154-192): every :ok read must sum to :total-amount and, unless negative-balances? is set, hold no negative balance."""

    def __init__(self, opts=None):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts, total, neg = _si_opts(test, self.opts)
        accts = set(accounts)
        reads = [op for op in ledger_to_bank(_indexed(history)) if H.client_op(op) and op["type"] == "ok" and op.get("f") == "read"]
        groups = {}
        for op in reads:
            e = check_op(accts, total, neg, op)
            if e is not None:
                groups.setdefault(e["type"], []).append(e)
        return _si_map(total, len(reads), groups)


class UnexpectedOps(jc.Checker):
    """unexpected-ops (:194-220): invokes never resolved, and fails, make the result :unknown."""

    def check(self, test, history, opts=None):
        h = [op for op in history if H.client_op(op)]
        out = {"valid?": True}
        if not h:
            return out
        end = h[-1].get("time")
        opens = [((end - op["time"]) / 1e6 if end is not None and op.get("time") is not None else None, op) for op in H.unmatched_invokes(h)]
        fails = [op for op in h if op["type"] == "fail"]
        if opens:
            out.update({"valid?": "unknown", "open-ops": opens[::-1]})
        if fails:
            out.update({"valid?": "unknown", "fail-ops": fails})
        return out


def _final_rows(history, f):
    return [op for op in history if H.client_op(op) and op_txn_f(op) == f and op["type"] == "ok" and op.get("final?")]


class LookupAllInvokedTransfers(jc.Checker):
    """lookup-transfers (:222-252): did every final lookup return every transfer that was invoked?"""

    def check(self, test, history, opts=None):
        invoked = set()
        for op in history:
            if H.client_op(op) and op_txn_f(op) == "t" and op["type"] == "invoke":
                invoked.update(m[1] for m in op["value"])
        suspect = [op for op in _final_rows(history, "l-t") if invoked - {m[1] for m in op["value"]}]
        out = {"valid?": True}
        if suspect:
            out.update({"valid?": False, "suspect-final-lookups": suspect})
        return out


def _distinct_values(ops):
    seen, out = set(), []
    for op in ops:
        k = _hashable(op["value"])
        if k not in seen:
            seen.add(k)
            out.append(op["value"])
    return out


class FinalReads(jc.Checker):
    """final-reads (:254-282): final reads and final lookups exist and are equal."""

    def check(self, test, history, opts=None):
        reads, lookups = _distinct_values(_final_rows(history, "r")), _distinct_values(_final_rows(history, "l-t"))
        out = {"valid?": True}
        if len(reads) != 1:
            out.update({"valid?": False, "unequal-final-reads": reads})
        if len(lookups) != 1:
            out.update({"valid?": False, "unequal-final-lookups": lookups})
        return out


# ---------------------------------------------------------------- the device route

_READ_KEYS = frozenset(("credits-posted", "debits-posted"))
_XFER_KEYS = frozenset(("debit-acct", "credit-acct", "amount"))


def _i64(x, what, i):
    if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)) or not _I64[0] <= x < _I64[1]:
        raise ValueError(f"op {i}: {what} {x!r} is not an int in int64 range")
    return int(x)


def _transfer_block(value):
    """the micro-ops of a long transfer / lookup value as (id, a, b, c, flags) arrays, None if any of them needs a closer look (a nil map,
    other keys, something that is no int64: the per-field path then says what)"""
    try:
        rows = [(m[1], d["debit-acct"], d["credit-acct"], d["amount"]) for m in value for d in (m[2],) if len(d) == 3]
        if len(rows) != len(value) or not all(type(x) is int for r in rows for x in r):
            return None
        arr = np.array(rows)
    except (TypeError, KeyError, OverflowError):
        return None
    if arr.dtype != np.int64 or arr.ndim != 2:
        return None
    return tuple(np.ascontiguousarray(arr[:, j]) for j in range(4)) + (np.zeros(len(rows), np.uint8),)


class LedgerColumns:
    """The client ops of a ledger history as the flat columns of tbc_ledger_in: per op index (its position in the history), type, kind
    (op->txn-f), flags (:final?) and its slice of the micro-op columns id, a, b, c, flags.  One plain pass that copies.  It applies no
    checker rule except the two the columns cannot express otherwise: an :ok :r value is a map after ledger->bank, so of several
    micro-ops with the same id in one read the last wins (in the first one's place); an op whose value is empty or nil has no first
    micro-op, so its kind is OTHER.  Only the ops a checker looks at -- :ok reads, invoked transfers, :ok lookups -- have their
    micro-ops copied; the others keep their kind and no micro-ops.

    `process` is the ops' :process (realtime pairs by it).

    ValueError: a :process outside int32 range; an id, an account, an amount or a posted sum that is not an int in int64 range (nil included); a micro-op map with other
    keys than the ones the columns hold; a :final? read that names an id twice (its raw vector and its map differ); a read whose
    sum of |credits| + |debits|, plus |total_amount|, reaches 2^63 (no device sum can wrap below that)."""

    def __init__(self, history, total_amount=0):
        total_amount = _i64(total_amount, "total-amount", -1)
        pos, type_, kind, flags, mop_n, proc = [], [], [], [], [], []
        ids, a_, b_, c_, mf = [], [], [], [], []
        chunks, n_mops = [], 0                      # the micro-ops so far as (id, a, b, c, flags) arrays; `ids` ... `mf` hold the tail

        def flush():
            nonlocal n_mops
            n_mops += len(ids)
            if ids:
                chunks.append(tuple(np.array(x, np.int64).reshape(-1) for x in (ids, a_, b_, c_)) + (np.array(mf, np.uint8),))
                for x in (ids, a_, b_, c_, mf):
                    x.clear()

        for i, op in enumerate(history):
            if not H.client_op(op):
                continue
            t = _TYPE.get(op.get("type"), N.LEDGER_T_INFO)
            f = op_txn_f(op)
            k = _KIND.get(f, N.LEDGER_K_OTHER)
            final = bool(op.get("final?"))
            n0 = n_mops + len(ids)
            if k == N.LEDGER_K_READ and t == N.LEDGER_T_OK:
                row, mag = {}, abs(total_amount)
                for mop in op["value"]:
                    ident, m = _i64(mop[1], "a read's id", i), mop[2]
                    if ident in row and final:
                        raise ValueError(f"op {i}: a :final? read names id {ident} twice")
                    if m is None:
                        row[ident] = (0, 0, N.LEDGER_M_NIL)
                        continue
                    if set(m) != _READ_KEYS:
                        raise ValueError(f"op {i}: a read's map has keys {sorted(m)!r}")
                    cr, db = _i64(m["credits-posted"], "credits-posted", i), _i64(m["debits-posted"], "debits-posted", i)
                    row[ident] = (cr, db, 0)
                for ident, (cr, db, fl) in row.items():
                    mag += abs(cr) + abs(db)
                    ids.append(ident); a_.append(cr); b_.append(db); c_.append(0); mf.append(fl)
                if mag >= _I64[1]:
                    raise ValueError(f"op {i}: the read's |credits| + |debits| + |total-amount| reaches 2^63")
            elif (k == N.LEDGER_K_TRANSFER and t == N.LEDGER_T_INVOKE) or (k == N.LEDGER_K_LOOKUP and t == N.LEDGER_T_OK):
                block = _transfer_block(op["value"]) if len(op["value"]) >= 64 else None
                if block is not None:               # (a long lookup whose micro-ops are all plain: one array, no per-field Python)
                    flush()
                    chunks.append(block)
                    n_mops += len(block[0])
                for mop in op["value"] if block is None else ():
                    ids.append(_i64(mop[1], "a transfer's id", i))
                    m = mop[2]
                    if m is None:
                        a_.append(0); b_.append(0); c_.append(0); mf.append(N.LEDGER_M_NIL)
                        continue
                    if set(m) != _XFER_KEYS:
                        raise ValueError(f"op {i}: a transfer's map has keys {sorted(m)!r}")
                    a_.append(_i64(m["debit-acct"], "debit-acct", i)); b_.append(_i64(m["credit-acct"], "credit-acct", i))
                    c_.append(_i64(m["amount"], "amount", i)); mf.append(0)
            pos.append(i); type_.append(t); kind.append(k); flags.append(N.LEDGER_F_FINAL if final else 0); mop_n.append(n_mops + len(ids) - n0)
            proc.append(op["process"])
        flush()
        self.total_amount = total_amount
        self.index = np.array(pos, np.uint32)
        self.type, self.kind, self.flags = np.array(type_, np.uint8), np.array(kind, np.uint8), np.array(flags, np.uint8)
        if any(not -(2 ** 31) <= p < 2 ** 31 for p in proc):
            raise ValueError("a :process is not an int in int32 range")
        self.process = np.array(proc, np.int32).reshape(-1)     # (pairing is by process: realtime)
        self.mop_off = np.concatenate([[0], np.cumsum(np.array(mop_n, np.int64))]).astype(np.uint64)
        cat = lambda j, dt: np.ascontiguousarray(np.concatenate([c[j] for c in chunks])) if chunks else np.zeros(0, dt)
        self.mop_id, self.mop_a, self.mop_b, self.mop_c = (cat(j, np.int64) for j in range(4))
        self.mop_flags = cat(4, np.uint8)
        ok = self.type == N.LEDGER_T_OK
        fin = (self.flags & N.LEDGER_F_FINAL) != 0
        # which op (position in the history) is which row of the outputs
        self.read_ops = self.index[ok & (self.kind == N.LEDGER_K_READ)]
        self.final_read_ops = self.index[ok & fin & (self.kind == N.LEDGER_K_READ)]
        self.final_lookup_ops = self.index[ok & fin & (self.kind == N.LEDGER_K_LOOKUP)]

    def __len__(self):
        return len(self.index)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def ledger_in(cols, accounts, negative_balances=False, device=0):
    """A tbc_ledger_in over a LedgerColumns (and the arrays it points into: keep them while the struct is used)."""
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    keep = {f: pad(np.ascontiguousarray(getattr(cols, f))) for f in ("index", "type", "kind", "flags", "mop_off", "mop_id", "mop_a", "mop_b", "mop_c", "mop_flags")}
    try:
        keep["accounts"] = pad(np.array(list(accounts), np.int64).reshape(-1))
    except (OverflowError, TypeError, ValueError):
        raise ValueError("an account is not an int in int64 range") from None
    s = N.LedgerIn()
    s.n_ops, s.device = len(cols), device
    s.index = _ptr(keep["index"], C.c_uint32)
    s.type, s.kind, s.flags = (_ptr(keep[f], C.c_uint8) for f in ("type", "kind", "flags"))
    s.mop_off = _ptr(keep["mop_off"], C.c_uint64)
    s.mop_id, s.mop_a, s.mop_b, s.mop_c = (_ptr(keep[f], C.c_int64) for f in ("mop_id", "mop_a", "mop_b", "mop_c"))
    s.mop_flags = _ptr(keep["mop_flags"], C.c_uint8)
    s.accounts, s.n_accounts, s.negative_balances = _ptr(keep["accounts"], C.c_int64), len(list(accounts)), int(bool(negative_balances))
    s.total_amount = cols.total_amount
    return s, keep


def summary_dict(s):
    d = {f: int(getattr(s, f)) for f, _ in N.LedgerSummary._fields_ if f not in ("errors", "reserved0")}
    d["errors"] = {ERROR_TYPES[k]: {f: int(getattr(s.errors[k], f)) for f in ("count", "first", "last", "worst")} for k in range(1, 5)}
    return d


def check_native(cols, accounts, negative_balances=False, device=0, call=None):
    """tbc_ledger_check over the columns -> the raw arrays and the summary (a dict).  call(in, out): another implementation of the entry
    point to fill `out` (the tests' emulator build of the same kernels)."""
    s, keep = ledger_in(cols, accounts, negative_balances, device)
    R, FR, FL = len(cols.read_ops), len(cols.final_read_ops), len(cols.final_lookup_ops)
    z = lambda n, dt: np.zeros(max(1, n), dt)
    arr = {"read_error": z(R, np.uint8), "read_total": z(R, np.int64), "read_badness": z(R, np.int64), "lookup_missing": z(FL, np.uint32),
           "final_read_unlike": z(FR, np.uint8), "final_lookup_unlike": z(FL, np.uint8)}
    ct = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.int64): C.c_int64, np.dtype(np.uint32): C.c_uint32}
    out = N.LedgerOut()
    for f, x in arr.items():
        setattr(out, f, _ptr(x, ct[x.dtype]))
    if call is None:
        N.check_status(N.lib().tbc_ledger_check(C.byref(s), C.byref(out)))
    else:
        call(s, out)
    del keep
    res = {f: x[:n] for (f, x), n in zip(arr.items(), (R, R, R, FL, FR, FL))}
    res["summary"] = summary_dict(out.summary)
    return res


def result_maps(history, cols, dev, accounts, negative_balances):
    """{"SI", "lookup-transfers", "final-reads"} as the host statement gives them, from tbc_ledger_check's arrays.  Ops are named from
    read and lookup numbers by index arrays; the handful of error maps the SI result shows, and the values of the rare invalid
    final rows, are taken from the history's ops."""
    s = dev["summary"]
    accts, total = set(accounts), cols.total_amount
    hist = _indexed(history) if any("index" not in op for op in history) else history

    def error_of(read):
        return check_op(accts, total, negative_balances, _bank_op(hist[int(cols.read_ops[read])]))

    errors = {}
    for k in range(1, 5):
        e = s["errors"][ERROR_TYPES[k]]
        if not e["count"]:
            continue
        m = {"count": e["count"], "first": error_of(e["first"]), "worst": error_of(e["worst"]), "last": error_of(e["last"])}
        if k == N.LEDGER_E_WRONG_TOTAL:
            m["lowest"], m["highest"] = error_of(s["lowest"]), error_of(s["highest"])
        errors[ERROR_TYPES[k]] = m
    # (insertion order as the host statement's group-by: by each type's first read)
    errors = dict(sorted(errors.items(), key=lambda kv: kv[1]["first"]["op"]["index"]))
    si = {"valid?": bool(s["valid_si"]), "read-count": s["read_count"], "error-count": s["error_count"],
          "first-error": error_of(s["first_error"]) if s["error_count"] else None, "errors": errors}
    lt = {"valid?": bool(s["valid_lookups"])}
    if s["suspect_lookups"]:
        lt["suspect-final-lookups"] = [history[int(i)] for i in cols.final_lookup_ops[dev["lookup_missing"] != 0]]
    fr = {"valid?": True}
    if s["n_final_reads"] == 0 or s["final_reads_unlike"]:
        fr.update({"valid?": False, "unequal-final-reads": _distinct_values(history[int(i)] for i in cols.final_read_ops)})
    if s["n_final_lookups"] == 0 or s["final_lookups_unlike"]:
        fr.update({"valid?": False, "unequal-final-lookups": _distinct_values(history[int(i)] for i in cols.final_lookup_ops)})
    return {"SI": si, "lookup-transfers": lt, "final-reads": fr}


def check_columns(history, opts=None, device=0):
    """columns -> tbc_ledger_check -> {"SI", "lookup-transfers", "final-reads"}: the host statement's three result maps, decided on the
    device.  opts: "accounts", "total-amount", "negative-balances?" (the reference's defaults).  NoDeviceError without a gfx950 device."""
    accounts, total, neg = _si_opts(None, opts)
    cols = LedgerColumns(history, total)
    return result_maps(history, cols, check_native(cols, accounts, neg, device), accounts, neg)


class _Shared:
    """ONE check_columns call per history for the three device members of a compose (they run concurrently: the first to ask computes,
    the others wait for it).  The result is dropped when all three have had it, so the checker holds on to no history.  There is no
    other route behind it: a history the columns cannot express raises LedgerColumns' ValueError, a missing device NoDeviceError."""

    MEMBERS = ("SI", "lookup-transfers", "final-reads")

    def __init__(self, opts):
        self.opts, self.lock, self.key, self.res, self.left = opts, threading.Lock(), None, None, 0

    def result(self, name, test, history, opts):
        with self.lock:
            if self.key is not history:
                o = dict(self.opts)
                o.update({k: v for k, v in (test or {}).items() if k in ("accounts", "total-amount")})
                self.key, self.res, self.left = None, None, 0
                self.res = check_columns(history, o, device=(opts or {}).get("device", 0))
                self.key, self.left = history, len(self.MEMBERS)
            res = self.res[name]
            self.left -= 1
            if self.left == 0:
                self.key, self.res = None, None
            return res


class _DeviceMember(jc.Checker):
    def __init__(self, shared, name):
        self.shared, self.name = shared, name

    def check(self, test, history, opts=None):
        return self.shared.result(self.name, test, history, opts)


class _Linear(jc.Checker):
    """The :linear member clj/patches/ledger.patch adds: linearizable against the bank model over ledger->bank of the history (a
    transfer's value is its map, as the shim's transfer-map takes it)."""

    def __init__(self, accounts, negative_balances):
        self.inner = jc.Linearizable({"model": M.bank(accounts, negative_balances)})

    def check(self, test, history, opts=None):
        bank = [dict(op, value=op["value"][0][2]) if H.client_op(op) and op.get("f") == "transfer" else op for op in ledger_to_bank(history)]
        return self.inner.check(test, bank, opts)


# ---------------------------------------------------------------- realtime bounds on posted counters

RT_KINDS = ("stale", "future", "regressed")
RT_FIELDS = ("credits-posted", "debits-posted")
_I64_MIN, _I64_MAX = -(2 ** 63), 2 ** 63 - 1


def _rt_opts(test, opts):
    """(accounts, {account: (init credits, init debits)}, ok-transfers-apply?) of a test map and the checker's options"""
    t = dict(opts or {})
    t.update({k: v for k, v in (test or {}).items() if k in ("accounts", "initial")})
    accounts = list(t.get("accounts") or range(1, 9))
    initial = t.get("initial") or {}
    init = {a: (initial.get(a, {}).get("credits-posted", 0), initial.get(a, {}).get("debits-posted", 0)) for a in accounts}
    apply_ok = (opts or {}).get("ok-transfers-apply?", True)
    return accounts, init, bool(True if apply_ok is None else apply_ok)


def _sat(x):
    return max(_I64_MIN, min(_I64_MAX, x))


def _read_mops(op):
    """the micro-ops of an :ok read as the columns hold them: (id, credits-posted, debits-posted, nil?), after ledger->bank's last-wins"""
    row = {}
    for _r, ident, m in op["value"]:
        row[ident] = (0, 0, True) if m is None else (m["credits-posted"], m["debits-posted"], False)
    return [(ident,) + v for ident, v in row.items()]


def _rt_model(history):
    """(transfers, reads) of a history.  A transfer: {"inv", "ret", "status", "mops": [(debit-acct, credit-acct, amount) | None]};
    a read: {"inv", "ret", "mops": [(id, credits, debits, nil?)]}."""
    pairs = H.pair_index(history)
    transfers, reads = [], []
    for i, op in enumerate(history):
        if not H.client_op(op):
            continue
        f = op_txn_f(op)
        if f == "t" and op["type"] == "invoke":
            j = pairs.get(i)
            status = "open" if j is None else (history[j]["type"] if history[j]["type"] in ("ok", "fail") else "info")
            mops = [None if m[2] is None else (m[2]["debit-acct"], m[2]["credit-acct"], m[2]["amount"]) for m in op["value"]]
            transfers.append({"inv": i, "ret": j, "status": status, "mops": mops})
        elif f == "r" and op["type"] == "ok":
            j = pairs.get(i)
            reads.append({"inv": -1 if j is None else j, "ret": i, "mops": _read_mops(op)})
    return transfers, reads


def _rt_ranges(amounts, n_transfer_mops, init):
    """the ranges under which no 64-bit sum can wrap (the module docstring's Ranges)"""
    for amount in amounts:
        if not 0 <= amount < 2 ** 31:
            raise ValueError(f"realtime: a transfer amount {amount!r} is not in [0, 2^31)")
    if n_transfer_mops >= 2 ** 31:
        raise ValueError("realtime: 2^31 or more transfer micro-ops")
    for a, cd in init.items():
        for x in cd:
            if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)) or not abs(x) < 2 ** 61:
                raise ValueError(f"realtime: initial value {x!r} of account {a!r} is not an int with |x| < 2^61")


def _rt_bounds_of(transfers, reads, accts, init, apply_ok, r):
    """Read r, micro-op by micro-op: None where it is not checked, else [(lo, hi, floor) of credits-posted, ... of debits-posted] --
    the three bounds exactly as the module docstring quantifies them."""
    R = reads[r]
    out = []
    for ident, cr, db, nil in R["mops"]:
        if nil or ident not in accts:
            out.append(None)
            continue
        per_field = []
        for x in (0, 1):                                      # credits-posted: the transfer's credit-acct; debits-posted: its debit-acct
            side = 1 if x == 0 else 0
            lo = hi = init[ident][x]
            for T in transfers:
                amount = sum(m[2] for m in T["mops"] if m is not None and m[side] == ident)
                if apply_ok and T["status"] == "ok" and T["ret"] < R["inv"]:
                    lo += amount
                if T["status"] != "fail" and T["inv"] < R["ret"]:
                    hi += amount
            floor = _I64_MIN
            for Q in reads:
                if Q["ret"] < R["inv"]:
                    for ident2, cr2, db2, nil2 in Q["mops"]:
                        if ident2 == ident and not nil2:
                            floor = max(floor, (cr2, db2)[x])
            per_field.append((lo, hi, floor))
        out.append(per_field)
    return out


def _rt_violations(R, bounds):
    """the violations of one read in the order the result map names them, as (micro-op, field, kind, miss, bound)"""
    out = []
    for j, (mop, b) in enumerate(zip(R["mops"], bounds)):
        if b is None:
            continue
        for x in (0, 1):
            v, (lo, hi, floor) = mop[1 + x], b[x]
            for k, (miss, bound) in enumerate(((lo - v, lo), (v - hi, hi), (floor - v, floor))):
                if miss > 0:
                    out.append((j, x, k, _sat(miss), bound))
    return out


def _rt_summary(bits, miss, foreign_sides, n_definite, n_possible, n_checked):
    """the summary of tbc_ledger_rt_summary (without ns_device and bytes_in) from the per-read arrays"""
    s = {"read_count": len(bits), "error_count": int(np.count_nonzero(bits)), "first_error": N.NO_OP, "valid": int(not bits.any()),
         "n_definite": n_definite, "n_possible": n_possible, "foreign_sides": foreign_sides, "bad_amounts": 0, "n_checked": n_checked, "errors": {}}
    if bits.any():
        s["first_error"] = int(np.flatnonzero(bits)[0])
    for k, kind in enumerate(RT_KINDS):
        has = np.flatnonzero(bits & (3 << (2 * k)))
        e = {"count": len(has), "first": N.NO_OP, "last": N.NO_OP, "worst": N.NO_OP}
        if len(has):
            e.update({"first": int(has[0]), "last": int(has[-1]), "worst": int(has[np.argmax(miss[has, k])])})      # (argmax: the earliest of equals)
        s["errors"][kind] = e
    return s


def realtime_host(history, opts=None):
    """The specification of the realtime bounds (module docstring), quantifier by quantifier; quadratic.  Per :ok read (LedgerColumns'
    read_ops numbering) "bits" and "miss" [stale, future, regressed]; per read micro-op "lo" "hi" "floor" [credits, debits], INT64_MIN where
    it is not checked; and the "summary" tbc_ledger_realtime gives."""
    accounts, init, apply_ok = _rt_opts(None, opts)
    accts = set(accounts)
    transfers, reads = _rt_model(history)
    counted = [T for T in transfers if T["status"] != "fail"]
    _rt_ranges([m[2] for T in counted for m in T["mops"] if m is not None], sum(len(T["mops"]) for T in counted), init)
    n_mops = sum(len(R["mops"]) for R in reads)
    bits, miss = np.zeros(len(reads), np.uint8), np.zeros((len(reads), 3), np.int64)
    lo, hi, floor = (np.full((n_mops, 2), _I64_MIN, np.int64) for _ in range(3))
    at = n_checked = 0
    for r, R in enumerate(reads):
        bounds = _rt_bounds_of(transfers, reads, accts, init, apply_ok, r)
        for j, b in enumerate(bounds):
            if b is not None:
                n_checked += 1
                for x in (0, 1):
                    lo[at + j, x], hi[at + j, x], floor[at + j, x] = b[x]
        for _j, x, k, m, _bound in _rt_violations(R, bounds):
            bits[r] |= 1 << (2 * k + x)
            miss[r, k] = max(miss[r, k], m)
        at += len(R["mops"])
    foreign = sum(2 if m is None else (m[0] not in accts) + (m[1] not in accts) for T in counted for m in T["mops"])
    return {"bits": bits, "miss": miss, "lo": lo, "hi": hi, "floor": floor,
            "summary": _rt_summary(bits, miss, foreign, sum(T["status"] == "ok" for T in transfers), len(counted), n_checked)}


def _rt_init_arrays(accounts, init):
    try:
        acct = np.array(list(accounts), np.int64).reshape(-1)
    except (OverflowError, TypeError, ValueError):
        raise ValueError("an account is not an int in int64 range") from None
    return acct, np.array([init[a][0] for a in accounts], np.int64).reshape(-1), np.array([init[a][1] for a in accounts], np.int64).reshape(-1)


def _expand(lo, n):
    """the micro-op numbers lo[k] .. lo[k] + n[k] - 1 of every row k in turn, and each one's row"""
    row = np.repeat(np.arange(len(n)), n)
    start = np.cumsum(n) - n
    return (lo[row] + (np.arange(len(row)) - start[row])).astype(np.int64), row


def _sat_sub(a, b):
    """a - b on int64 arrays, saturating"""
    with np.errstate(over="ignore"):
        d = a - b
    over = ((a < 0) != (b < 0)) & ((d < 0) != (a < 0))
    return np.where(over, np.where(a < 0, _I64_MIN, _I64_MAX), d)


def _partner_rows(cols):
    """pairing (knossos.history.pair_index) over a LedgerColumns: per row the row of its completion / invocation, -1 if it has none.
    Along one process an invocation is completed by the very next op when that is a completion."""
    n = len(cols)
    order = np.argsort(cols.process, kind="stable")
    p, t = cols.process[order], cols.type[order]
    match = (p[1:] == p[:-1]) & (t[:-1] == N.LEDGER_T_INVOKE) & (t[1:] != N.LEDGER_T_INVOKE) if n > 1 else np.zeros(0, bool)
    partner = np.full(n, -1, np.int64)
    partner[order[1:][match]] = order[:-1][match]
    partner[order[:-1][match]] = order[1:][match]
    return partner


def realtime_numpy_columns(cols, accounts, init, apply_ok=True):
    """realtime_host's arrays from a LedgerColumns in O(n log n): a stable sort by (account, position), cumsum / maximum.accumulate along it,
    and searchsorted for every read micro-op.  The reference at sizes the quadratic statement cannot reach."""
    T_INV, T_OK, T_FAIL = N.LEDGER_T_INVOKE, N.LEDGER_T_OK, N.LEDGER_T_FAIL
    _rt_ranges([], 0, init)
    acct, init_c, init_d = _rt_init_arrays(accounts, init)
    index, typ, kind = cols.index.astype(np.int64), cols.type, cols.kind
    off = cols.mop_off.astype(np.int64)
    partner = _partner_rows(cols)
    tr = np.flatnonzero((typ == T_INV) & (kind == N.LEDGER_K_TRANSFER))
    status = np.where(partner[tr] >= 0, typ[partner[tr]], T_INV)                 # (T_INV: open)
    ret = np.where(partner[tr] >= 0, index[partner[tr]], -1)
    poss = tr[status != T_FAIL]
    keep = status == T_OK
    defi, defi_pos = tr[keep][np.argsort(ret[keep], kind="stable")], np.sort(ret[keep])
    sort_acct = np.sort(acct)
    perm = np.argsort(acct, kind="stable")
    init_x = (init_c[perm], init_d[perm])
    A = len(acct)

    def number(ids):
        k = np.searchsorted(sort_acct, ids)
        k[k == A] = 0
        return np.where(sort_acct[k] == ids, k, -1) if A else np.full(len(ids), -1, np.int64)

    def entries(rows, pos):
        """per field x (credits, debits) the entries (account number, position, amount) of the transfers `rows`, sorted by (account, position)"""
        m, row = _expand(off[rows], off[rows + 1] - off[rows])
        nil = (cols.mop_flags[m] & N.LEDGER_M_NIL) != 0
        out, foreign = [], 0
        for ids in (cols.mop_b[m], cols.mop_a[m]):
            a = np.where(nil, -1, number(ids))
            ok = a >= 0
            foreign += int(np.count_nonzero(~ok))
            comp = a[ok] * (1 << 32) + pos[row][ok]
            o = np.argsort(comp, kind="stable")
            out.append((comp[o], np.concatenate([[0], np.cumsum(cols.mop_c[m][ok][o])])))
        return out, foreign, m[~nil]

    def prefix(lists, x, a, position):
        comp, cs = lists[x]
        return cs[np.searchsorted(comp, a * (1 << 32) + position, "left")] - cs[np.searchsorted(comp, a * (1 << 32), "left")]

    poss_lists, foreign, poss_m = entries(poss, index[poss])
    _rt_ranges(cols.mop_c[poss_m][(cols.mop_c[poss_m] < 0) | (cols.mop_c[poss_m] >= 2 ** 31)][:1].tolist(), int((off[poss + 1] - off[poss]).sum()), {})
    defi_lists, _, _ = entries(defi, defi_pos)
    # the reads
    rd = np.flatnonzero((typ == T_OK) & (kind == N.LEDGER_K_READ))
    r_ret, r_inv = index[rd], np.where(partner[rd] >= 0, index[np.maximum(partner[rd], 0)], -1)
    m, row = _expand(off[rd], off[rd + 1] - off[rd])
    a = np.where((cols.mop_flags[m] & N.LEDGER_M_NIL) != 0, -1, number(cols.mop_id[m]))
    chk = a >= 0
    ac, inv, rt = a[chk], r_inv[row][chk], r_ret[row][chk]
    lo, hi, floor = (np.full((len(m), 2), _I64_MIN, np.int64) for _ in range(3))
    bits, miss = np.zeros(len(rd), np.uint8), np.zeros((len(rd), 3), np.int64)
    comp = ac * (1 << 32) + rt
    o = np.argsort(comp, kind="stable")
    comp_s = comp[o]
    for x, vals in enumerate((cols.mop_a[m][chk], cols.mop_b[m][chk])):
        lo_x = init_x[x][ac] + (prefix(defi_lists, x, ac, np.maximum(inv, 0)) if apply_ok else 0)
        hi_x = init_x[x][ac] + prefix(poss_lists, x, ac, rt)
        # running maximum per account: values as ranks, an account's ranks above every earlier account's
        fl_x = np.full(len(ac), _I64_MIN, np.int64)
        if len(ac):
            sorted_vals = np.sort(vals)
            rank = np.searchsorted(sorted_vals, vals[o], "left")
            run = np.maximum.accumulate(ac[o] * len(ac) + rank) - ac[o] * len(ac)
            k, k0 = np.searchsorted(comp_s, ac * (1 << 32) + np.maximum(inv, 0), "left"), np.searchsorted(comp_s, ac * (1 << 32), "left")
            fl_x = np.where(k > k0, sorted_vals[run[np.maximum(k, 1) - 1]], _I64_MIN)
        lo[chk, x], hi[chk, x], floor[chk, x] = lo_x, hi_x, fl_x
        for k, ms in enumerate((_sat_sub(lo_x, vals), _sat_sub(vals, hi_x), _sat_sub(fl_x, vals))):
            bad = ms > 0
            np.bitwise_or.at(bits, row[chk][bad], np.uint8(1 << (2 * k + x)))
            np.maximum.at(miss[:, k], row[chk][bad], ms[bad])
    return {"bits": bits, "miss": miss, "lo": lo, "hi": hi, "floor": floor,
            "summary": _rt_summary(bits, miss, foreign, len(defi), len(poss), int(np.count_nonzero(chk)))}


def realtime_numpy(history, opts=None):
    """realtime_host(history, opts), in O(n log n) (realtime_numpy_columns over the history's LedgerColumns)."""
    accounts, init, apply_ok = _rt_opts(None, opts)
    return realtime_numpy_columns(LedgerColumns(history), accounts, init, apply_ok)


def _rt_named(hist, model, accts, init, apply_ok, r):
    """{"op", "violations"} of read r"""
    transfers, reads = model
    R = reads[r]
    vs = _rt_violations(R, _rt_bounds_of(transfers, reads, accts, init, apply_ok, r))
    return {"op": hist[R["ret"]], "violations": [{"type": RT_KINDS[k], "account": R["mops"][j][0], "field": RT_FIELDS[x], "value": R["mops"][j][1 + x], "bound": b}
                                                for j, x, k, _m, b in vs]}


def _rt_map(history, summary, accounts, init, apply_ok):
    """the realtime result map from a summary (the host statement's or the device's): the named reads recomputed from the history"""
    if not summary["error_count"]:                      # (no read to name: no pass over the history)
        return {"valid?": True, "read-count": summary["read_count"], "error-count": 0, "first-error": None, "errors": {}}
    hist = _indexed(history) if any("index" not in op for op in history) else history
    model, accts = _rt_model(history), set(accounts)
    named = lambda r: _rt_named(hist, model, accts, init, apply_ok, r)
    errors = {kind: {"count": e["count"], "first": named(e["first"]), "worst": named(e["worst"]), "last": named(e["last"])}
              for kind, e in summary["errors"].items() if e["count"]}
    return {"valid?": bool(summary["valid"]), "read-count": summary["read_count"], "error-count": summary["error_count"],
            "first-error": named(summary["first_error"]) if summary["error_count"] else None, "errors": errors}


class RealtimeBounds(jc.Checker):
    """realtime: every counter an :ok read returns lies within what real time allows (module docstring) -- a necessary condition for
    strict serializability.  opts: "accounts", "initial" {account: {"credits-posted": c, "debits-posted": d}}, "ok-transfers-apply?"."""

    def __init__(self, opts=None):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts, init, apply_ok = _rt_opts(test, self.opts)
        o = dict(self.opts, accounts=accounts, initial={a: dict(zip(RT_FIELDS, cd)) for a, cd in init.items()})
        return _rt_map(history, realtime_host(history, o)["summary"], accounts, init, apply_ok)


def ledger_rt_in(cols, accounts, init, apply_ok=True, device=0):
    """A tbc_ledger_rt_in over a LedgerColumns (and the arrays it points into).  ValueError: the Ranges of the module docstring that the
    columns show -- an amount of a transfer that did not fail outside [0, 2^31), 2^31 transfer micro-ops, an initial value of 2^61."""
    T = (cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER)
    _rt_ranges([], int((cols.mop_off[1:][T].astype(np.int64) - cols.mop_off[:-1][T].astype(np.int64)).sum()), init)
    s, keep = ledger_in(cols, accounts, False, device)
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    _acct, init_c, init_d = _rt_init_arrays(accounts, init)
    keep.update({"process": pad(np.ascontiguousarray(cols.process)), "init_c": pad(init_c), "init_d": pad(init_d)})
    r = N.LedgerRtIn()
    r.ledger = s
    r.process = _ptr(keep["process"], C.c_int32)
    r.init_credits, r.init_debits = _ptr(keep["init_c"], C.c_int64), _ptr(keep["init_d"], C.c_int64)
    r.ok_transfers_apply = int(bool(apply_ok))
    return r, keep


def rt_summary_dict(s):
    d = {f: int(getattr(s, f)) for f, _ in N.LedgerRtSummary._fields_ if f != "errors"}
    d["errors"] = {RT_KINDS[k]: {f: int(getattr(s.errors[k], f)) for f in ("count", "first", "last", "worst")} for k in range(3)}
    return d


def check_realtime_native(cols, accounts, init, apply_ok=True, device=0, call=None):
    """tbc_ledger_realtime over the columns -> realtime_host's arrays and the summary (with ns_device and bytes_in).  call(in, out): another
    implementation of the entry point (the tests' emulator build of the same kernels).  An amount out of range is the device's to find
    (TBC_ERR_UNSUPPORTED): ValueError here too."""
    s, keep = ledger_rt_in(cols, accounts, init, apply_ok, device)
    R = len(cols.read_ops)
    rd = (cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ)
    M = int((cols.mop_off[1:][rd].astype(np.int64) - cols.mop_off[:-1][rd].astype(np.int64)).sum())
    arr = {"rt_bits": np.zeros(max(1, R), np.uint8), "rt_miss": np.zeros((max(1, R), 3), np.int64)}
    arr.update({f: np.zeros((max(1, M), 2), np.int64) for f in ("mop_lo", "mop_hi", "mop_floor")})
    out = N.LedgerRtOut()
    out.rt_bits = _ptr(arr["rt_bits"], C.c_uint8)
    for f in ("rt_miss", "mop_lo", "mop_hi", "mop_floor"):
        setattr(out, f, _ptr(arr[f], C.c_int64))
    if call is None:
        st = N.lib().tbc_ledger_realtime(C.byref(s), C.byref(out))
        if st == N.ERR_UNSUPPORTED:
            raise ValueError("realtime: " + N.lib().tbc_last_error().decode())
        N.check_status(st)
    else:
        call(s, out)
    del keep
    return {"bits": arr["rt_bits"][:R], "miss": arr["rt_miss"][:R], "lo": arr["mop_lo"][:M], "hi": arr["mop_hi"][:M], "floor": arr["mop_floor"][:M],
            "summary": rt_summary_dict(out.summary)}


def realtime_result_map(history, cols, dev, accounts, init, apply_ok=True):
    """RealtimeBounds' result map from tbc_ledger_realtime's summary; only the handful of reads it names are recomputed on the host (a
    valid history: none, and no pass over it).  `cols` names the reads the summary numbers -- cols.read_ops, which _rt_model restates --
    and is taken for the symmetry with result_maps; the map needs nothing else of it."""
    assert dev["summary"]["read_count"] == len(cols.read_ops)
    return _rt_map(history, dev["summary"], accounts, init, apply_ok)


class _RealtimeDevice(jc.Checker):
    """the realtime member on the device route: columns -> tbc_ledger_realtime -> RealtimeBounds' map.  No host route behind it."""

    def __init__(self, opts):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts, init, apply_ok = _rt_opts(test, self.opts)
        cols = LedgerColumns(history)
        dev = check_realtime_native(cols, accounts, init, apply_ok, device=(opts or {}).get("device", 0))
        return realtime_result_map(history, cols, dev, accounts, init, apply_ok)


# ---------------------------------------------------------------- snapshot order of the reads

SNAP_PARTIAL, SNAP_SKEWED = 1, 2


def _snap_accounts(test, opts):
    t = dict(opts or {})
    t.update({k: v for k, v in (test or {}).items() if k == "accounts"})
    return list(t.get("accounts") or range(1, 9))


def _snap_vectors(history, accounts):
    """per :ok read (LedgerColumns' read_ops numbering) its vector {counter: value} over the counters it checks, and their history indexes"""
    pos = {a: k for k, a in enumerate(accounts)}
    vectors, index = [], []
    for i, op in enumerate(history):
        if H.client_op(op) and op_txn_f(op) == "r" and op["type"] == "ok":
            v = {}
            for ident, cr, db, nil in _read_mops(op):
                if not nil and ident in pos:
                    v[2 * pos[ident]], v[2 * pos[ident] + 1] = cr, db
            if sum(abs(x) for x in v.values()) >= 2 ** 63:
                raise ValueError(f"snapshots: op {i}: the read's |credits| + |debits| reach 2^63")
            vectors.append(v)
            index.append(i)
    return vectors, index


def _snap_summary(count, flags, n_checked, n_candidates):
    """the summary of tbc_ledger_snap_summary (without ns_device and bytes_in) from the per-read arrays"""
    has = np.flatnonzero(count)
    e = {"count": len(has), "first": N.NO_OP, "last": N.NO_OP, "worst": N.NO_OP}
    if len(has):
        e.update({"first": int(has[0]), "last": int(has[-1]), "worst": int(has[np.argmax(count[has])])})       # (argmax: the earliest of equals)
    return {"read_count": len(count), "n_partial": int(np.count_nonzero(flags & SNAP_PARTIAL)), "valid": int(not len(has)), "bad_values": 0,
            "skewed": e, "n_candidates": n_candidates, "n_checked": n_checked, "n_pairs": int(count.astype(np.int64).sum()) // 2}


def snapshots_vectors_host(vectors, n_accounts):
    """The specification of the snapshot order (module docstring) over vectors {counter: value}, pair by pair; O(R^2 C).  Per read "count",
    "first", "key" [below, above] and "flags", and the "summary" tbc_ledger_snapshots gives."""
    R = len(vectors)
    below = lambda a, b: sorted(c for c in a if c in b and a[c] < b[c])
    complete = [len(v) == 2 * n_accounts for v in vectors]
    count, first = np.zeros(R, np.uint32), np.full(R, N.NO_OP, np.uint32)
    key, flags = np.full((R, 2), N.NO_OP, np.uint32), np.zeros(R, np.uint8)
    with_complete = [False] * R
    for i in range(R):
        for j in range(R):
            if i != j and below(vectors[i], vectors[j]) and below(vectors[j], vectors[i]):
                count[i] += 1
                with_complete[i] = with_complete[i] or complete[j]
                if first[i] == N.NO_OP:
                    first[i] = j
                    key[i] = below(vectors[i], vectors[j])[0], below(vectors[j], vectors[i])[0]
        flags[i] = (0 if complete[i] else SNAP_PARTIAL) | (SNAP_SKEWED if count[i] else 0)
    n_candidates = sum(1 for i in range(R) if not complete[i] or with_complete[i])
    return {"count": count, "first": first, "key": key, "flags": flags,
            "summary": _snap_summary(count, flags, sum(len(v) // 2 for v in vectors), n_candidates)}


def snapshots_host(history, opts=None):
    """snapshots_vectors_host over the history's :ok reads (LedgerColumns' read_ops numbering).  opts: "accounts"."""
    accounts = _snap_accounts(None, opts)
    return snapshots_vectors_host(_snap_vectors(history, accounts)[0], len(accounts))


def snapshots_dense_numpy(V, K):
    """The sort-and-scan statement over dense rows: V [R][C] int64 values, K [R][C] bool, which are checked (C = 2 x accounts).  The
    complete reads sorted by (sum, read number); for i before j in that order skewed(i, j) <=> some v_i[c] > v_j[c], so the exclusive prefix
    maximum and suffix minimum per counter flag exactly the complete reads skewed with a complete read; those and the partial reads are
    the candidates, and only they are compared with every read.  What the device is held to, n_candidates included."""
    R, C = V.shape
    complete = K.all(axis=1)
    near = np.flatnonzero((np.abs(V.astype(np.float64)) * K).sum(axis=1) >= 2.0 ** 62)       # (the few rows worth exact arithmetic)
    if any(sum(abs(int(x)) for x in V[r][K[r]]) >= 2 ** 63 for r in near):
        raise ValueError("snapshots: a read's |credits| + |debits| reach 2^63")
    count, first = np.zeros(R, np.int64), np.full(R, N.NO_OP, np.int64)
    key = np.full((R, 2), N.NO_OP, np.uint32)
    flagged = np.zeros(R, bool)
    full = np.flatnonzero(complete)
    if len(full) and C:
        order = full[np.lexsort((full, V[full].sum(axis=1)))]
        S = V[order]
        before = np.vstack([np.full((1, C), _I64_MIN, np.int64), np.maximum.accumulate(S, axis=0)[:-1]])
        after = np.vstack([np.minimum.accumulate(S[::-1], axis=0)[::-1][1:], np.full((1, C), _I64_MAX, np.int64)])
        flagged[order] = (before > S).any(axis=1) | (after < S).any(axis=1)
    cand = flagged | ~complete
    for i in np.flatnonzero(cand):
        both = K & K[i]
        skewed = (both & (V[i] < V)).any(axis=1) & (both & (V[i] > V)).any(axis=1)
        partners = np.flatnonzero(skewed)
        count[i] += len(partners)
        if len(partners):
            first[i] = min(first[i], partners[0])
        others = partners[~cand[partners]]                       # partners that are no candidates: nobody else counts these pairs
        count[others] += 1
        first[others] = np.minimum(first[others], i)
    for i in np.flatnonzero(count):
        j = first[i]
        both = K[i] & K[j]
        key[i] = np.flatnonzero(both & (V[i] < V[j]))[0], np.flatnonzero(both & (V[i] > V[j]))[0]
    flags = (np.where(complete, 0, SNAP_PARTIAL) | np.where(count > 0, SNAP_SKEWED, 0)).astype(np.uint8)
    count = count.astype(np.uint32)
    return {"count": count, "first": first.astype(np.uint32), "key": key, "flags": flags,
            "summary": _snap_summary(count, flags, int(K.sum()) // 2, int(np.count_nonzero(cand)))}


def _snap_dense(cols, accounts):
    """the :ok reads of a LedgerColumns as dense rows (V, K) over the counters of `accounts`"""
    try:
        acct = np.array(list(accounts), np.int64).reshape(-1)
    except (OverflowError, TypeError, ValueError):
        raise ValueError("an account is not an int in int64 range") from None
    A = len(acct)
    off = cols.mop_off.astype(np.int64)
    rd = np.flatnonzero((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ))
    m, row = _expand(off[rd], off[rd + 1] - off[rd])
    V, K = np.zeros((len(rd), 2 * A), np.int64), np.zeros((len(rd), 2 * A), bool)
    if A and len(m):
        perm = np.argsort(acct, kind="stable")
        k = np.minimum(np.searchsorted(acct[perm], cols.mop_id[m]), A - 1)
        chk = (acct[perm][k] == cols.mop_id[m]) & ((cols.mop_flags[m] & N.LEDGER_M_NIL) == 0)
        c = 2 * perm[k][chk]
        V[row[chk], c], V[row[chk], c + 1] = cols.mop_a[m][chk], cols.mop_b[m][chk]
        K[row[chk], c] = K[row[chk], c + 1] = True
    return V, K


def snapshots_numpy(history, opts=None):
    """snapshots_host(history, opts) by sort and scan (snapshots_dense_numpy over the history's LedgerColumns)."""
    accounts = _snap_accounts(None, opts)
    return snapshots_dense_numpy(*_snap_dense(LedgerColumns(history), accounts))


def _snap_map(history, read_ops, res, accounts):
    """the snapshots result map from the per-read arrays and the summary (the host statement's or the device's)"""
    s = res["summary"]
    out = {"valid?": bool(s["valid"]), "exact?": s["n_partial"] == 0, "read-count": s["read_count"], "partial-count": s["n_partial"],
           "skewed-count": s["skewed"]["count"], "pair-count": s["n_pairs"], "first": None, "worst": None, "last": None}
    if not s["skewed"]["count"]:                        # (no read to name: no pass over the history)
        return out
    hist = _indexed(history) if any("index" not in op for op in history) else history
    counter = lambda c: [accounts[int(c) // 2], RT_FIELDS[int(c) % 2]]

    def named(r):
        return {"op": hist[int(read_ops[r])], "skew-count": int(res["count"][r]), "with": hist[int(read_ops[int(res["first"][r])])],
                "below": counter(res["key"][r][0]), "above": counter(res["key"][r][1])}

    out.update({k: named(s["skewed"][k]) for k in ("first", "worst", "last")})
    return out


class SnapshotOrder(jc.Checker):
    """snapshots: no two :ok reads are skewed -- each below the other on some posted counter (module docstring, "Snapshot order").  With
    every read complete this and RealtimeBounds' regressed bit are the whole cycle search over monotonic-key and realtime edges
    ("exact?"); with partial reads it is sound but not complete.  opts: "accounts"."""

    def __init__(self, opts=None):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts = _snap_accounts(test, self.opts)
        vectors, index = _snap_vectors(history, accounts)
        return _snap_map(history, index, snapshots_vectors_host(vectors, len(accounts)), accounts)


def ledger_snap_in(cols, accounts, device=0):
    """The tbc_ledger_in tbc_ledger_snapshots takes over a LedgerColumns (and the arrays it points into)."""
    return ledger_in(cols, accounts, False, device)


def snap_summary_dict(s):
    d = {f: int(getattr(s, f)) for f, _ in N.LedgerSnapSummary._fields_ if f not in ("skewed", "reserved0")}
    d["skewed"] = {f: int(getattr(s.skewed, f)) for f in ("count", "first", "last", "worst")}
    return d


def check_snapshots_native(cols, accounts, device=0, call=None):
    """tbc_ledger_snapshots over the columns -> snapshots_host's arrays and the summary (with ns_device and bytes_in).  call(in, out): another
    implementation of the entry point (the tests' emulator build of the same kernels).  A read out of range is the device's to find
    (TBC_ERR_UNSUPPORTED): ValueError here too."""
    s, keep = ledger_snap_in(cols, accounts, device)
    R = len(cols.read_ops)
    arr = {"skew_count": np.zeros(max(1, R), np.uint32), "skew_first": np.zeros(max(1, R), np.uint32),
           "skew_key": np.zeros((max(1, R), 2), np.uint32), "snap_flags": np.zeros(max(1, R), np.uint8)}
    out = N.LedgerSnapOut()
    for f in ("skew_count", "skew_first", "skew_key"):
        setattr(out, f, _ptr(arr[f], C.c_uint32))
    out.snap_flags = _ptr(arr["snap_flags"], C.c_uint8)
    if call is None:
        st = N.lib().tbc_ledger_snapshots(C.byref(s), C.byref(out))
        if st == N.ERR_UNSUPPORTED:
            raise ValueError("snapshots: " + N.lib().tbc_last_error().decode())
        N.check_status(st)
    else:
        call(s, out)
    del keep
    return {"count": arr["skew_count"][:R], "first": arr["skew_first"][:R], "key": arr["skew_key"][:R], "flags": arr["snap_flags"][:R],
            "summary": snap_summary_dict(out.summary)}


def snapshots_result_map(history, cols, dev, accounts):
    """SnapshotOrder's result map from tbc_ledger_snapshots' arrays and summary: the three reads it names come from the history by index
    (a valid history: none, and no pass over it)."""
    assert dev["summary"]["read_count"] == len(cols.read_ops)
    return _snap_map(history, cols.read_ops, dev, list(accounts))


class _SnapshotDevice(jc.Checker):
    """the snapshots member on the device route: columns -> tbc_ledger_snapshots -> SnapshotOrder's map.  No host route behind it."""

    def __init__(self, opts):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts = _snap_accounts(test, self.opts)
        cols = LedgerColumns(history)
        dev = check_snapshots_native(cols, accounts, device=(opts or {}).get("device", 0))
        return snapshots_result_map(history, cols, dev, accounts)


# ---------------------------------------------------------------- cycles over monotonic and realtime edges, partial reads included

CYC_PARTIAL, CYC_ON_CYCLE, CYC_CORE = 1, 2, 4
CYCLES_MAX_CORE = N.LEDGER_CYCLES_MAX_CORE    # TBC_LEDGER_CYCLES_MAX_CORE
CYC_ARRAYS = ("scc", "flags")


def _cyc_model(history, accounts):
    """per :ok read its vector {counter: value}, its history index, inv and ret (the snapshot and the realtime rules' own statements)"""
    vectors, index = _snap_vectors(history, accounts)
    reads = _rt_model(history)[1]
    assert [R["ret"] for R in reads] == index
    return vectors, index, [R["inv"] for R in reads], [R["ret"] for R in reads]


def _cyc_edge(vectors, inv, ret, a, b):
    """the edge a -> b of the rules: None, or ("realtime",) / ("monotonic", counter) -- realtime named first, then the least counter"""
    if ret[a] < inv[b]:
        return ("realtime",)
    below = sorted(c for c in vectors[a] if c in vectors[b] and vectors[a][c] < vectors[b][c])
    return ("monotonic", below[0]) if below else None


def _tarjan(n, succ):
    """the strongly connected components of 0 .. n-1 (succ[v]: v's successors), iteratively: comp[v] = the least vertex of v's component"""
    index, low, on, stack, comp = [None] * n, [0] * n, [False] * n, [], list(range(n))
    count = 0
    for root in range(n):
        if index[root] is not None:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = count
                count += 1
                stack.append(v)
                on[v] = True
            for k2 in range(k, len(succ[v])):
                w = succ[v][k2]
                if index[w] is None:
                    work.append((v, k2 + 1))
                    work.append((w, 0))
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            else:
                if low[v] == index[v]:
                    members = []
                    while True:
                        w = stack.pop()
                        on[w] = False
                        members.append(w)
                        if w == v:
                            break
                    for w in members:
                        comp[w] = min(members)
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
    return comp


def _cyc_summary(scc, flags, n_checked, closure_rounds):
    """the summary of tbc_ledger_cycles_summary (without ns_device and bytes_in) from the per-read arrays"""
    on = np.flatnonzero(flags & CYC_ON_CYCLE)
    labels, sizes = np.unique(scc[on], return_counts=True)
    s = {"read_count": len(scc), "n_partial": int(np.count_nonzero(flags & CYC_PARTIAL)), "n_core": int(np.count_nonzero(flags & CYC_CORE)),
         "n_on_cycle": len(on), "n_components": len(labels), "first": N.NO_OP, "largest": N.NO_OP, "largest_size": 0, "valid": int(not len(on)),
         "closure_rounds": closure_rounds, "bad_values": 0, "n_checked": n_checked}
    if len(on):
        s.update({"first": int(on[0]), "largest": int(labels[np.argmax(sizes)]), "largest_size": int(sizes.max())})     # (argmax: the earliest of equals)
    return s


def cycles_vectors_host(vectors, inv, ret, n_accounts):
    """The specification of the cycle search (module docstring) over vectors {counter: value} with inv and ret: the explicit graph, edge by
    edge, and Tarjan; O(R^2 C).  Per read "scc" and "flags", and the "summary" tbc_ledger_cycles gives but for closure_rounds, which only
    the reduction has (None here)."""
    R = len(vectors)
    succ = [[b for b in range(R) if b != a and _cyc_edge(vectors, inv, ret, a, b)] for a in range(R)]
    comp = _tarjan(R, succ)
    size = np.bincount(np.array(comp, np.int64), minlength=R) if R else np.zeros(0, np.int64)
    below = lambda a, b: any(c in b and a[c] < b[c] for c in a)
    complete = [len(v) == 2 * n_accounts for v in vectors]
    total = [sum(v.values()) for v in vectors]
    U = [complete[i] and not any(complete[j] and below(vectors[i], vectors[j]) and below(vectors[j], vectors[i]) for j in range(R)) for i in range(R)]
    rt_flagged = [U[i] and any(U[j] and ret[j] < inv[i] and total[j] > total[i] for j in range(R)) for i in range(R)]
    scc, flags = np.full(R, N.NO_OP, np.uint32), np.zeros(R, np.uint8)
    for r in range(R):
        on = size[comp[r]] >= 2
        if on:
            scc[r] = comp[r]
        flags[r] = (0 if complete[r] else CYC_PARTIAL) | (CYC_ON_CYCLE if on else 0) | (0 if U[r] and not rt_flagged[r] else CYC_CORE)
    return {"scc": scc, "flags": flags, "summary": _cyc_summary(scc, flags, sum(len(v) // 2 for v in vectors), None)}


def cycles_host(history, opts=None):
    """cycles_vectors_host over the history's :ok reads (LedgerColumns' read_ops numbering).  opts: "accounts"."""
    accounts = _snap_accounts(None, opts)
    vectors, _index, inv, ret = _cyc_model(history, accounts)
    return cycles_vectors_host(vectors, inv, ret, len(accounts))


def _bool_square(A):
    """A | A.A over booleans"""
    f = A.astype(np.float32)
    return A | ((f @ f) > 0)


def cycles_dense_numpy(V, K, inv, ret):
    """The REDUCTION the device computes, over dense rows (V, K as snapshots_dense_numpy takes them) with inv and ret [R] (ret ascending:
    reads are numbered in history order).  The clean reads -- complete, comparable with every complete read, not rt-flagged -- form a
    chain of CLASSES (the ranks of their distinct sums) along which every edge runs upwards, so they are never laid out as a graph: a core
    read P keeps s_out (the least class it has an edge to), s_in (the greatest class with an edge to it) and whether a monotonic edge
    realises each; the m x m matrix over the core has the direct edges and the edges mediated by clean reads; boolean squaring closes
    it; a clean read joins the core component whose (lo, hi) descriptors enclose it.  Held to cycles_host array by array."""
    R, C = V.shape
    inv, ret = np.asarray(inv, np.int64), np.asarray(ret, np.int64)
    near = np.flatnonzero((np.abs(V.astype(np.float64)) * K).sum(axis=1) >= 2.0 ** 62)       # (the few rows worth exact arithmetic)
    if any(sum(abs(int(x)) for x in V[r][K[r]]) >= 2 ** 63 for r in near):
        raise ValueError("cycles: a read's |credits| + |debits| reach 2^63")
    complete = K.all(axis=1)
    total = V.sum(axis=1) if C else np.zeros(R, np.int64)
    flagged = np.zeros(R, bool)
    full = np.flatnonzero(complete)
    if len(full) and C:
        order = full[np.lexsort((full, total[full]))]
        S = V[order]
        before = np.vstack([np.full((1, C), _I64_MIN, np.int64), np.maximum.accumulate(S, axis=0)[:-1]])
        after = np.vstack([np.minimum.accumulate(S[::-1], axis=0)[::-1][1:], np.full((1, C), _I64_MAX, np.int64)])
        flagged[order] = (before > S).any(axis=1) | (after < S).any(axis=1)
    U = complete & ~flagged
    # rt-flagged: the greatest sum over the reads of U that returned before this one was invoked is above its own
    n_before = np.searchsorted(ret, inv, side="left")                      # reads with ret < inv(r)
    pmax = np.maximum.accumulate(np.where(U, total, _I64_MIN)) if R else np.zeros(0, np.int64)
    best = np.where(n_before > 0, pmax[np.maximum(n_before, 1) - 1], _I64_MIN) if R else pmax
    clean = U & ~(best > total)
    core = np.flatnonzero(~clean)
    cl = np.flatnonzero(clean)
    m = len(core)
    scc, on = np.full(R, N.NO_OP, np.int64), np.zeros(R, bool)
    rounds = 0
    if m:
        # the classes, and one vector per class
        sums, first_of, cls_of = np.unique(total[cl], return_index=True, return_inverse=True) if len(cl) else (np.zeros(0, np.int64),) * 3
        n_cls = len(sums)
        Vc = V[cl[first_of]] if n_cls else np.zeros((0, C), np.int64)
        cls = np.full(R, -1, np.int64)
        cls[cl] = cls_of
        INF = n_cls                                                               # +inf of s_out; -1 is the -inf of s_in
        Vp, Kp = V[core], K[core]
        mono_out, mono_in = np.full(m, INF, np.int64), np.full(m, -1, np.int64)
        for c in range(C):
            up = np.searchsorted(Vc[:, c], Vp[:, c], side="right")                # the least class above P on c
            dn = np.searchsorted(Vc[:, c], Vp[:, c], side="left") - 1            # the greatest class below P on c
            mono_out = np.where(Kp[:, c], np.minimum(mono_out, up), mono_out)
            mono_in = np.where(Kp[:, c], np.maximum(mono_in, dn), mono_in)
        by_inv = cl[np.argsort(inv[cl], kind="stable")]
        sufmin = np.minimum.accumulate(cls[by_inv][::-1])[::-1] if len(cl) else np.zeros(0, np.int64)
        at = np.searchsorted(inv[by_inv], ret[core], side="right")              # the first clean read invoked after P returned
        rt_out = np.where(at < len(cl), np.append(sufmin, INF)[at], INF)
        premax = np.maximum.accumulate(cls[cl]) if len(cl) else np.zeros(0, np.int64)
        nb = np.searchsorted(ret[cl], inv[core], side="left")                   # the clean reads that returned before P was invoked
        rt_in = np.where(nb > 0, np.append(premax, -1)[nb - 1], -1)
        s_out, s_in = np.minimum(mono_out, rt_out), np.maximum(mono_in, rt_in)
        m_out, m_in = (mono_out == s_out) & (s_out < INF), (mono_in == s_in) & (s_in >= 0)
        A = np.zeros((m, m), bool)
        for i in range(m):
            both = Kp & Kp[i]
            A[i] = (both & (Vp[i] < Vp)).any(axis=1) | (ret[core[i]] < inv[core])
            A[i] |= (s_out[i] < s_in) | ((s_out[i] == s_in) & (m_out[i] | m_in))
        while True:
            B = _bool_square(A)
            rounds += 1
            if (B == A).all():
                break
            A = B
        S = A & A.T
        np.fill_diagonal(S, True)
        rep = S.argmax(axis=1)                                                   # the least core read of P's component
        for k in np.flatnonzero(rep == np.arange(m)):
            mem = np.flatnonzero(rep == k)
            lo, hi = s_out[mem].min(), s_in[mem].max()
            at_lo, at_hi = mem[s_out[mem] == lo], mem[s_in[mem] == hi]
            lo_mono, hi_mono = m_out[at_lo].any(), m_in[at_hi].any()
            lo_ret, hi_inv = ret[core[at_lo]].min(), inv[core[at_hi]].max()
            inside = ((cls[cl] > lo) | ((cls[cl] == lo) & (lo_mono | (inv[cl] > lo_ret)))) & ((cls[cl] < hi) | ((cls[cl] == hi) & (hi_mono | (ret[cl] < hi_inv))))
            assert not on[cl[inside]].any()                                      # (components are disjoint: a clean read joins one)
            members = np.concatenate([core[mem], cl[inside]])
            if len(members) >= 2:
                scc[members], on[members] = members.min(), True
    flags = (np.where(complete, 0, CYC_PARTIAL) | np.where(on, CYC_ON_CYCLE, 0) | np.where(clean, 0, CYC_CORE)).astype(np.uint8)
    scc = scc.astype(np.uint32)
    return {"scc": scc, "flags": flags, "summary": _cyc_summary(scc, flags, int(K.sum()) // 2, rounds)}


def _cyc_times(cols):
    """inv and ret of the :ok reads of a LedgerColumns (pairing by process, as the realtime rules state it)"""
    rd = np.flatnonzero((cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_READ))
    partner = _partner_rows(cols)[rd]
    index = cols.index.astype(np.int64)
    return np.where(partner >= 0, index[np.maximum(partner, 0)], -1), index[rd]


def cycles_numpy(history, opts=None):
    """cycles_host(history, opts) by the reduction (cycles_dense_numpy over the history's LedgerColumns), closure_rounds included."""
    accounts = _snap_accounts(None, opts)
    cols = LedgerColumns(history)
    return cycles_dense_numpy(*_snap_dense(cols, accounts), *_cyc_times(cols))


def _cyc_witness(vectors, inv, ret, members, label):
    """one shortest cycle through `label` inside its component, by BFS: [(from, to, edge)]"""
    inside = set(members)
    prev, frontier = {}, [label]
    while frontier:
        nxt = []
        for a in frontier:
            for b in sorted(inside):
                if b != a and b not in prev and _cyc_edge(vectors, inv, ret, a, b):
                    prev[b] = a
                    if b == label:
                        path = [label]
                        while True:
                            path.append(prev[path[-1]])
                            if path[-1] == label:
                                break
                        path.reverse()
                        return [(a2, b2, _cyc_edge(vectors, inv, ret, a2, b2)) for a2, b2 in zip(path, path[1:])]
                    nxt.append(b)
        frontier = nxt
    return []


def _cyc_map(history, res, accounts):
    """the cycles result map from the per-read arrays and the summary (the host statement's or the device's)"""
    s = res["summary"]
    out = {"valid?": bool(s["valid"]), "exact?": True, "read-count": s["read_count"], "partial-count": s["n_partial"], "core-count": s["n_core"],
           "on-cycle-count": s["n_on_cycle"], "component-count": s["n_components"], "largest-size": s["largest_size"], "components": [], "witness": None}
    if not s["n_on_cycle"]:                             # (no read to name: no pass over the history)
        return out
    hist = _indexed(history) if any("index" not in op for op in history) else history
    vectors, index, inv, ret = _cyc_model(history, accounts)
    scc = res["scc"]
    labels = np.unique(scc[scc != N.NO_OP])
    for label in labels[:10]:
        members = np.flatnonzero(scc == label)
        out["components"].append({"label": hist[index[int(label)]], "size": len(members), "ops": [hist[index[int(r)]] for r in members[:10]]})
    members = np.flatnonzero(scc == labels[0])
    if len(members) <= 4096:
        counter = lambda c: [accounts[int(c) // 2], RT_FIELDS[int(c) % 2]]
        steps = []
        for a, b, e in _cyc_witness(vectors, inv, ret, [int(r) for r in members], int(labels[0])):
            step = {"from": hist[index[a]], "to": hist[index[b]], "type": e[0]}
            if e[0] == "monotonic":
                step.update({"key": counter(e[1]), "value": vectors[a][e[1]], "value'": vectors[b][e[1]]})
            steps.append(step)
        out["witness"] = steps
    return out


class CycleSearch(jc.Checker):
    """cycles: the graph of monotonic-key and realtime edges over the :ok reads is acyclic, partial reads included (module docstring,
    "Cycle search") -- the host statement: the explicit graph and Tarjan.  opts: "accounts"."""

    def __init__(self, opts=None):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts = _snap_accounts(test, self.opts)
        vectors, _index, inv, ret = _cyc_model(history, accounts)
        return _cyc_map(history, cycles_vectors_host(vectors, inv, ret, len(accounts)), accounts)


def cyc_summary_dict(s):
    return {f: int(getattr(s, f)) for f, _ in N.LedgerCyclesSummary._fields_ if f != "reserved0"}


def check_cycles_native(cols, accounts, device=0, call=None):
    """tbc_ledger_cycles over the columns -> cycles_host's arrays and the summary (with closure_rounds, ns_device and bytes_in).
    call(in, out) -> status: another implementation of the entry point (the tests' emulator build of the same kernels).  A read out of
    range is the device's to find: ValueError here too.  A core above TBC_LEDGER_CYCLES_MAX_CORE: {"unsupported": True, "summary"} with
    n_core filled and no arrays."""
    init = {a: (0, 0) for a in accounts}
    s, keep = ledger_rt_in(cols, accounts, init, True, device)
    R = len(cols.read_ops)
    arr = {"scc": np.zeros(max(1, R), np.uint32), "cyc_flags": np.zeros(max(1, R), np.uint8)}
    out = N.LedgerCyclesOut()
    out.scc, out.cyc_flags = _ptr(arr["scc"], C.c_uint32), _ptr(arr["cyc_flags"], C.c_uint8)
    st = N.lib().tbc_ledger_cycles(C.byref(s), C.byref(out)) if call is None else call(s, out)
    del keep
    summary = cyc_summary_dict(out.summary)
    if st == N.ERR_UNSUPPORTED and not summary["bad_values"]:                # (the only other refusal the device makes: the core is above the cap)
        return {"unsupported": True, "summary": summary}
    if st == N.ERR_UNSUPPORTED:
        raise ValueError("cycles: " + (N.lib().tbc_last_error().decode() if call is None else "reads hold counters whose magnitudes add up to 2^63 or more"))
    if call is None:
        N.check_status(st)
    else:
        assert st == 0, st
    return {"scc": arr["scc"][:R], "flags": arr["cyc_flags"][:R], "summary": summary}


def cycles_result_map(history, cols, dev, accounts):
    """CycleSearch's result map from tbc_ledger_cycles' arrays and summary; the components it names and the witness come from the history
    on the host (a valid history: none, and no pass over it).  Above the cap: "valid?" "unknown"."""
    assert dev["summary"]["read_count"] == len(cols.read_ops)
    if dev.get("unsupported"):
        return {"valid?": "unknown", "searched?": False, "n-core": dev["summary"]["n_core"]}
    return _cyc_map(history, dev, list(accounts))


class _CycleDevice(jc.Checker):
    """the cycles member on the device route: columns -> tbc_ledger_cycles -> CycleSearch's map.  No host route behind it."""

    def __init__(self, opts):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts = _snap_accounts(test, self.opts)
        cols = LedgerColumns(history)
        dev = check_cycles_native(cols, accounts, device=(opts or {}).get("device", 0))
        return cycles_result_map(history, cols, dev, accounts)


# ---------------------------------------------------------------- the journal audit of the lookups

JN_KINDS = ("unknown", "altered", "repeated", "failed", "early", "lost", "vanished", "ahead", "behind")       # by TBC_LEDGER_JN_*
JN_RECORD_KINDS = ("failed", "early", "lost", "vanished")
JN_ARRAYS = ("entry_bits", "lk_counts", "lk_present", "lk_vector", "rd_bits", "rd_first", "xfer_present", "xfer_early", "xfer_lost",
             "xfer_vanished", "xfer_flags")


def _jn_model(history):
    """(transfer micro-ops, lookups) of a history.  A transfer micro-op: {"id", "fields": (debit-acct, credit-acct, amount) | None, "inv",
    "ret", "status"} (its owner's); a lookup: {"inv", "ret", "entries": [(id, fields | None)]}."""
    pairs = H.pair_index(history)
    fields = lambda m: None if m[2] is None else (m[2]["debit-acct"], m[2]["credit-acct"], m[2]["amount"])
    xfers, lookups = [], []
    for i, op in enumerate(history):
        if not H.client_op(op):
            continue
        f, j = op_txn_f(op), pairs.get(i)
        if f == "t" and op["type"] == "invoke":
            status = "open" if j is None else (history[j]["type"] if history[j]["type"] in ("ok", "fail") else "info")
            xfers.extend({"id": m[1], "fields": fields(m), "inv": i, "ret": j, "status": status} for m in op["value"])
        elif f == "l-t" and op["type"] == "ok":
            lookups.append({"inv": -1 if j is None else j, "ret": i, "entries": [(m[1], fields(m)) for m in op["value"]]})
    return xfers, lookups


def _jn_ranges(amounts, n_xfer_mops, entries_per_lookup, init):
    for amount in amounts:
        if not 0 <= amount < 2 ** 31:
            raise ValueError(f"journal: a journalled transfer's amount {amount!r} is not in [0, 2^31)")
    if n_xfer_mops >= 2 ** 31:
        raise ValueError("journal: 2^31 or more transfer micro-ops")
    if any(n >= 2 ** 31 for n in entries_per_lookup):
        raise ValueError("journal: a lookup of 2^31 or more entries")
    for a, cd in init.items():
        for x in cd:
            if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)) or not abs(x) < 2 ** 61:
                raise ValueError(f"journal: initial value {x!r} of account {a!r} is not an int with |x| < 2^61")


def _jn_summary(res, n_records, n_reinvoked, foreign_sides, n_checked):
    """the summary of tbc_ledger_journal_summary (without ns_device and bytes_in) from the arrays"""
    counts = res["lk_counts"]
    s = {"n_lookups": len(counts), "n_xfer_mops": len(res["xfer_flags"]), "n_records": n_records, "n_reinvoked": n_reinvoked,
         "foreign_sides": foreign_sides, "bad_amounts": 0, "read_count": len(res["rd_bits"]), "n_entries": len(res["entry_bits"]),
         "n_checked": n_checked, "errors": {}, "totals": {}}
    for k, kind in enumerate(JN_KINDS):
        has = np.flatnonzero(counts[:, k])
        e = {"count": len(has), "first": N.NO_OP, "last": N.NO_OP, "worst": N.NO_OP}
        if len(has):
            e.update({"first": int(has[0]), "last": int(has[-1]), "worst": int(has[np.argmax(counts[has, k])])})     # (argmax: the earliest of equals)
        s["errors"][kind], s["totals"][kind] = e, int(counts[:, k].astype(np.int64).sum())
    s["valid"] = int(not any(s["totals"].values()))
    return s


def journal_host(history, opts=None):
    """The specification of the journal audit (module docstring), plain loops, one rule a line.  The arrays of tbc_ledger_journal_out by
    name (JN_ARRAYS) and the "summary"."""
    accounts, init, apply_ok = _rt_opts(None, opts)
    pos = {a: k for k, a in enumerate(accounts)}
    xfers, lookups = _jn_model(history)
    _transfers, reads = _rt_model(history)
    record = {}
    for m, x in enumerate(xfers):
        record.setdefault(x["id"], m)                                   # the first micro-op with the id
    is_record = [record[x["id"]] == m for m, x in enumerate(xfers)]
    _jn_ranges([x["fields"][2] for m, x in enumerate(xfers) if is_record[m] and x["fields"] is not None], len(xfers),
               [len(L["entries"]) for L in lookups], init)
    M, NL, R, C = len(xfers), len(lookups), len(reads), 2 * len(accounts)
    entry_bits = []
    counts, present_n, vector = np.zeros((NL, 9), np.uint32), np.zeros(NL, np.uint32), np.zeros((NL, C), np.int64)
    x_present, x_early, x_lost, x_vanished = (np.zeros(M, np.uint32) for _ in range(4))
    present = []
    for l, L in enumerate(lookups):
        here = set()
        for ident, fields in L["entries"]:
            if ident not in record:
                entry_bits.append(1); counts[l, 0] += 1                 # UNKNOWN
                continue
            rec = xfers[record[ident]]
            altered = fields is None or rec["fields"] is None or fields != rec["fields"]
            entry_bits.append(2 if altered else 0); counts[l, 1] += altered         # ALTERED
            counts[l, 2] += record[ident] in here                       # REPEATED
            here.add(record[ident])
        present.append(here)
        present_n[l] = len(here)
        J = {c: init[accounts[c // 2]][c % 2] for c in range(C)}
        for m, x in enumerate(xfers):
            if not is_record[m]:
                continue
            if m in here:
                x_present[m] += 1
                failed, early = x["status"] == "fail", x["inv"] > L["ret"]
                counts[l, 3] += failed; counts[l, 4] += early; x_early[m] += early
                if x["fields"] is not None:                             # BOOKS
                    debit, credit, amount = x["fields"]
                    if credit in pos:
                        J[2 * pos[credit]] += amount
                    if debit in pos:
                        J[2 * pos[debit] + 1] += amount
            else:
                lost = apply_ok and x["status"] == "ok" and x["ret"] < L["inv"]
                vanished = any(lookups[k]["ret"] < L["inv"] and m in present[k] for k in range(l))
                counts[l, 5] += lost; counts[l, 6] += vanished; x_lost[m] += lost; x_vanished[m] += vanished
        vector[l] = [J[c] for c in range(C)]
    rd_bits, rd_first = np.zeros(R, np.uint8), np.full((R, 2), N.NO_OP, np.uint32)
    n_checked = 0
    for r, Rd in enumerate(reads):
        checked = [(ident, cr, db) for ident, cr, db, nil in Rd["mops"] if not nil and ident in pos]
        n_checked += len(checked)
        for l, L in enumerate(lookups):
            ahead = Rd["ret"] < L["inv"] and any(v > vector[l, 2 * pos[a] + x] for a, *cd in checked for x, v in enumerate(cd))
            behind = L["ret"] < Rd["inv"] and any(v < vector[l, 2 * pos[a] + x] for a, *cd in checked for x, v in enumerate(cd))
            for k, hit in enumerate((ahead, behind)):
                if hit:
                    counts[l, 7 + k] += 1
                    rd_bits[r] |= 1 << k
                    rd_first[r, k] = min(rd_first[r, k], l)
    flags = np.array([(0 if is_record[m] else 1) | (2 if x["fields"] is None else 0) for m, x in enumerate(xfers)], np.uint8).reshape(-1)
    foreign = sum(2 if x["fields"] is None else (x["fields"][0] not in pos) + (x["fields"][1] not in pos) for m, x in enumerate(xfers) if is_record[m])
    res = {"entry_bits": np.array(entry_bits, np.uint8).reshape(-1), "lk_counts": counts, "lk_present": present_n, "lk_vector": vector,
           "rd_bits": rd_bits, "rd_first": rd_first, "xfer_present": x_present, "xfer_early": x_early, "xfer_lost": x_lost,
           "xfer_vanished": x_vanished, "xfer_flags": flags}
    res["summary"] = _jn_summary(res, sum(is_record), M - sum(is_record), foreign, n_checked)
    return res


def journal_numpy_columns(cols, accounts, init, apply_ok=True):
    """journal_host's arrays from a LedgerColumns, vectorised: the records by np.unique, a lookups x transfer-micro-ops presence matrix,
    the reads as the dense rows of the snapshot statement.  What the device is held to."""
    T_INV, T_OK, T_FAIL = N.LEDGER_T_INVOKE, N.LEDGER_T_OK, N.LEDGER_T_FAIL
    acct, init_c, init_d = _rt_init_arrays(accounts, init)
    A, C2 = len(acct), 2 * len(acct)
    index, typ, kind = cols.index.astype(np.int64), cols.type, cols.kind
    off = cols.mop_off.astype(np.int64)
    partner = _partner_rows(cols)
    p_index = np.where(partner >= 0, index[np.maximum(partner, 0)], -1)
    # the transfer micro-ops and their owners
    tr = np.flatnonzero((typ == T_INV) & (kind == N.LEDGER_K_TRANSFER))
    xm, xrow = _expand(off[tr], off[tr + 1] - off[tr])
    M = len(xm)
    x_id, x_nil = cols.mop_id[xm], (cols.mop_flags[xm] & N.LEDGER_M_NIL) != 0
    x_inv, x_ret = index[tr][xrow], p_index[tr][xrow]
    x_status = np.where(partner[tr] >= 0, typ[np.maximum(partner[tr], 0)], T_INV)[xrow]
    uniq, first_idx, inverse = np.unique(x_id, return_index=True, return_inverse=True)
    is_record = first_idx[inverse.reshape(-1)] == np.arange(M) if M else np.zeros(0, bool)
    # the lookups and their entries
    lk = np.flatnonzero((typ == T_OK) & (kind == N.LEDGER_K_LOOKUP))
    NL = len(lk)
    l_ret, l_inv = index[lk], p_index[lk]
    em, erow = _expand(off[lk], off[lk + 1] - off[lk])
    _jn_ranges(cols.mop_c[xm][is_record & ~x_nil][(cols.mop_c[xm][is_record & ~x_nil] < 0) | (cols.mop_c[xm][is_record & ~x_nil] >= 2 ** 31)][:1].tolist(),
               M, (off[lk + 1] - off[lk]).tolist(), init)
    e_id = cols.mop_id[em]
    at = np.minimum(np.searchsorted(uniq, e_id), max(len(uniq) - 1, 0))
    known = uniq[at] == e_id if M else np.zeros(len(em), bool)
    rec = first_idx[at] if M else np.zeros(len(em), np.int64)
    e_nil = (cols.mop_flags[em] & N.LEDGER_M_NIL) != 0
    xs = xm[rec] if M else em
    differ = e_nil | x_nil[rec] | (cols.mop_a[em] != cols.mop_a[xs]) | (cols.mop_b[em] != cols.mop_b[xs]) | (cols.mop_c[em] != cols.mop_c[xs]) if M else known
    entry_bits = np.where(known, np.where(differ, 2, 0), 1).astype(np.uint8)
    counts = np.zeros((NL, 9), np.uint32)
    counts[:, 0] = np.bincount(erow[~known], minlength=NL)
    counts[:, 1] = np.bincount(erow[known & differ], minlength=NL)
    P = np.zeros((NL, M), bool)
    P[erow[known], rec[known]] = True
    present_n = P.sum(axis=1).astype(np.uint32)
    counts[:, 2] = np.bincount(erow[known], minlength=NL) - present_n
    absent = ~P & is_record
    seen = P.any(axis=0)
    seen_ret = np.where(seen, l_ret[np.argmax(P, axis=0)] if NL else 0, np.iinfo(np.int64).max)       # (lookups are numbered by ret: the first that shows it has the least)
    failed, early = P & (x_status == T_FAIL), P & (x_inv[None, :] > l_ret[:, None])
    lost = absent & (x_status == T_OK) & (x_ret[None, :] < l_inv[:, None]) & bool(apply_ok)
    vanished = absent & (seen_ret[None, :] < l_inv[:, None])
    for k, what in ((3, failed), (4, early), (5, lost), (6, vanished)):
        counts[:, k] = what.sum(axis=1)
    # the books
    perm = np.argsort(acct, kind="stable")

    def counter(ids, x):
        k = np.minimum(np.searchsorted(acct[perm], ids), max(A - 1, 0))
        return np.where(acct[perm][k] == ids, 2 * perm[k] + x, -1) if A else np.full(len(ids), -1, np.int64)

    cc, dc = counter(cols.mop_b[xm], 0), counter(cols.mop_a[xm], 1)
    moves = is_record & ~x_nil
    vector = np.zeros((NL, C2), np.int64)
    vector[:, 0::2], vector[:, 1::2] = init_c, init_d
    amount = cols.mop_c[xm]
    for l in range(NL):
        for side in (cc, dc):
            m = np.flatnonzero(P[l] & moves & (side >= 0))
            np.add.at(vector[l], side[m], amount[m])
    foreign = int(2 * np.count_nonzero(is_record & x_nil) + np.count_nonzero(moves & (cc < 0)) + np.count_nonzero(moves & (dc < 0)))
    # the reads against the books
    V, K = _snap_dense(cols, accounts)
    rd = np.flatnonzero((typ == T_OK) & (kind == N.LEDGER_K_READ))
    r_ret, r_inv = index[rd], p_index[rd]
    R = len(rd)
    rd_bits, rd_first = np.zeros(R, np.uint8), np.full((R, 2), N.NO_OP, np.uint32)
    for l in range(NL - 1, -1, -1):                                     # (descending: the least lookup number is written last)
        ahead = (r_ret < l_inv[l]) & (K & (V > vector[l])).any(axis=1)
        behind = (l_ret[l] < r_inv) & (K & (V < vector[l])).any(axis=1)
        for k, hit in enumerate((ahead, behind)):
            counts[l, 7 + k] = np.count_nonzero(hit)
            rd_bits[hit] |= np.uint8(1 << k)
            rd_first[hit, k] = l
    x_flags = (np.where(is_record, 0, 1) | np.where(x_nil, 2, 0)).astype(np.uint8)
    res = {"entry_bits": entry_bits, "lk_counts": counts, "lk_present": present_n, "lk_vector": vector, "rd_bits": rd_bits, "rd_first": rd_first,
           "xfer_present": P.sum(axis=0).astype(np.uint32) * is_record.astype(np.uint32), "xfer_early": early.sum(axis=0).astype(np.uint32),
           "xfer_lost": lost.sum(axis=0).astype(np.uint32), "xfer_vanished": vanished.sum(axis=0).astype(np.uint32), "xfer_flags": x_flags}
    res["summary"] = _jn_summary(res, int(np.count_nonzero(is_record)), int(M - np.count_nonzero(is_record)), foreign, int(K.sum()) // 2)
    return res


def journal_numpy(history, opts=None):
    """journal_host(history, opts), vectorised (journal_numpy_columns over the history's LedgerColumns)."""
    accounts, init, apply_ok = _rt_opts(None, opts)
    return journal_numpy_columns(LedgerColumns(history), accounts, init, apply_ok)


def _jn_lookup_ops(cols):
    """which op (position in the history) is which lookup of the journal audit"""
    return cols.index[(cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_LOOKUP)]


def _jn_map(history, res):
    """the journal result map from the arrays and the summary (the host statement's or the device's): per kind count, total, and first,
    last, worst as the lookup ops; for the record kinds up to 10 offending ids"""
    s = res["summary"]
    out = {"valid?": bool(s["valid"]), "lookup-count": s["n_lookups"], "entry-count": s["n_entries"], "record-count": s["n_records"],
           "reinvoked-count": s["n_reinvoked"], "errors": {}}
    if s["valid"]:                                      # (nothing to name: no pass over the history)
        return out
    hist = _indexed(history) if any("index" not in op for op in history) else history
    xfers, lookups = _jn_model(history)
    failed = np.array([x["status"] == "fail" for x in xfers], bool).reshape(-1)
    offending = {"failed": (res["xfer_present"] > 0) & failed, "early": res["xfer_early"] > 0, "lost": res["xfer_lost"] > 0,
                 "vanished": res["xfer_vanished"] > 0}
    for kind in JN_KINDS:
        e = s["errors"][kind]
        if not e["count"]:
            continue
        m = {"count": e["count"], "total": s["totals"][kind]}
        m.update({k: hist[lookups[e[k]]["ret"]] for k in ("first", "last", "worst")})
        if kind in JN_RECORD_KINDS:
            m["ids"] = [xfers[int(i)]["id"] for i in np.flatnonzero(offending[kind])[:10]]
        out["errors"][kind] = m
    return out


class JournalAudit(jc.Checker):
    """journal: every :ok lookup audited entry by entry against the transfers as invoked, against real time and against the balances the
    reads returned (module docstring, "Journal audit").  opts: those of RealtimeBounds."""

    def __init__(self, opts=None):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts, init, _apply_ok = _rt_opts(test, self.opts)
        o = dict(self.opts, accounts=accounts, initial={a: dict(zip(RT_FIELDS, cd)) for a, cd in init.items()})
        return _jn_map(history, journal_host(history, o))


def jn_summary_dict(s):
    d = {f: int(getattr(s, f)) for f, _ in N.LedgerJournalSummary._fields_ if f not in ("errors", "totals")}
    d["errors"] = {JN_KINDS[k]: {f: int(getattr(s.errors[k], f)) for f in ("count", "first", "last", "worst")} for k in range(9)}
    d["totals"] = {JN_KINDS[k]: int(s.totals[k]) for k in range(9)}
    return d


def journal_shapes(cols):
    """(entries, lookups, reads, transfer micro-ops) of a LedgerColumns: what sizes tbc_ledger_journal's output arrays"""
    n = (cols.mop_off[1:].astype(np.int64) - cols.mop_off[:-1].astype(np.int64))
    lk = (cols.type == N.LEDGER_T_OK) & (cols.kind == N.LEDGER_K_LOOKUP)
    tr = (cols.type == N.LEDGER_T_INVOKE) & (cols.kind == N.LEDGER_K_TRANSFER)
    return int(n[lk].sum()), int(np.count_nonzero(lk)), len(cols.read_ops), int(n[tr].sum())


def journal_out(cols, n_accounts):
    """A tbc_ledger_journal_out over fresh arrays sized for the columns: (out, {name: array}, {name: true shape})"""
    E, NL, R, M = journal_shapes(cols)
    shape = {"entry_bits": (E,), "lk_counts": (NL, 9), "lk_present": (NL,), "lk_vector": (NL, 2 * n_accounts), "rd_bits": (R,), "rd_first": (R, 2),
             "xfer_present": (M,), "xfer_early": (M,), "xfer_lost": (M,), "xfer_vanished": (M,), "xfer_flags": (M,)}
    dtype = {"entry_bits": np.uint8, "rd_bits": np.uint8, "xfer_flags": np.uint8, "lk_vector": np.int64}
    arr = {f: np.zeros(max(1, int(np.prod(shape[f]))), dtype.get(f, np.uint32)) for f in JN_ARRAYS}
    ct = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.int64): C.c_int64, np.dtype(np.uint32): C.c_uint32}
    out = N.LedgerJournalOut()
    for f, x in arr.items():
        setattr(out, f, _ptr(x, ct[x.dtype]))
    return out, arr, shape


def check_journal_native(cols, accounts, init, apply_ok=True, device=0, call=None):
    """tbc_ledger_journal over the columns -> journal_host's arrays and the summary (with ns_device and bytes_in).  call(in, out): another
    implementation of the entry point (the tests' emulator build of the same kernels).  An amount out of range is the device's to find
    (TBC_ERR_UNSUPPORTED): ValueError here too."""
    s, keep = ledger_rt_in(cols, accounts, init, apply_ok, device)
    out, arr, shape = journal_out(cols, len(list(accounts)))
    if call is None:
        st = N.lib().tbc_ledger_journal(C.byref(s), C.byref(out))
        if st == N.ERR_UNSUPPORTED:
            raise ValueError("journal: " + N.lib().tbc_last_error().decode())
        N.check_status(st)
    else:
        call(s, out)
    del keep
    res = {f: arr[f][:int(np.prod(shape[f]))].reshape(shape[f]) for f in JN_ARRAYS}
    res["summary"] = jn_summary_dict(out.summary)
    return res


def journal_result_map(history, cols, dev):
    """JournalAudit's result map from tbc_ledger_journal's arrays and summary: the lookups it names come from the history (a valid
    history: none, and no pass over it)."""
    assert dev["summary"]["n_lookups"] == len(_jn_lookup_ops(cols))
    return _jn_map(history, dev)


class _JournalDevice(jc.Checker):
    """the journal member on the device route: columns -> tbc_ledger_journal -> JournalAudit's map.  No host route behind it."""

    def __init__(self, opts):
        self.opts = dict(opts or {})

    def check(self, test, history, opts=None):
        accounts, init, apply_ok = _rt_opts(test, self.opts)
        cols = LedgerColumns(history)
        dev = check_journal_native(cols, accounts, init, apply_ok, device=(opts or {}).get("device", 0))
        return journal_result_map(history, cols, dev)


def test(opts=None, linear=False, realtime=False, device_route=True, snapshots=False, journal=False, cycles=False):
    """The ledger test map (tests/ledger.clj:341-369) without generators: accounts, max-transfer, total-amount and the composed checker
    -- SI, lookup-transfers, final-reads, unexpected-ops, with linear=True the member clj/patches/ledger.patch adds, and with
    realtime=True the member "realtime" (RealtimeBounds; opts "initial", "ok-transfers-apply?") and with snapshots=True the member
    "snapshots" (SnapshotOrder) and with journal=True the member "journal" (JournalAudit; realtime's opts) and with cycles=True the member "cycles"
    (CycleSearch), each on the device or as the host statement according to device_route.
    device_route=True (the default: the whole call measured 1.7-1.8 s against the host statement's 6.6-6.7 s on a ledger of 64 workers and 50k
    transfers, profiles/NOTES_ledger.md) answers the first three from one check_columns call; False runs the host statement."""
    opts = dict(opts if opts is not None else {"negative-balances?": False})
    opts["max-transfer"] = opts.get("max-transfer") or 5
    opts["total-amount"] = opts.get("total-amount") or 0
    opts["accounts"] = list(opts.get("accounts") or range(1, 9))
    if device_route:
        shared = _Shared(opts)
        members = {name: _DeviceMember(shared, name) for name in _Shared.MEMBERS}
    else:
        members = {"SI": BankChecker(opts), "lookup-transfers": LookupAllInvokedTransfers(), "final-reads": FinalReads()}
    members["unexpected-ops"] = UnexpectedOps()
    if realtime:
        members["realtime"] = _RealtimeDevice(opts) if device_route else RealtimeBounds(opts)
    if snapshots:
        members["snapshots"] = _SnapshotDevice(opts) if device_route else SnapshotOrder(opts)
    if journal:
        members["journal"] = _JournalDevice(opts) if device_route else JournalAudit(opts)
    if cycles:
        members["cycles"] = _CycleDevice(opts) if device_route else CycleSearch(opts)
    if linear:
        members["linear"] = _Linear(opts["accounts"], bool(opts.get("negative-balances?", False)))
    return dict(opts, checker=jc.compose(members))

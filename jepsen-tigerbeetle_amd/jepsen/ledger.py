"""tigerbeetle.tests.ledger -- the ledger workload's checkers (the reference's tests/ledger.clj:89-282, composed at :363-367).

Two statements of the same checkers:

* the HOST statement, plain Python written for clarity: `ledger_to_bank`, `BankChecker` (:SI), `UnexpectedOps`,
  `LookupAllInvokedTransfers`, `FinalReads`.  It is the specification the device route is tested against.
* the DEVICE route: `LedgerColumns` flattens the client ops into the columns of tbc_ledger_in (include/tbcheck.h), `check_columns`
  hands them to tbc_ledger_check (csrc/ledger_*.h) and builds the same three result maps from the arrays that come back.
  `unexpected-ops` returns ops and is O(ops): it stays on the host.

`test()` gives the workload's map with the composed checker; with `device_route=True` its SI, lookup-transfers and final-reads members
answer from ONE `check_columns` call.  :plot is not built.

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

    ValueError: an id, an account, an amount or a posted sum that is not an int in int64 range (nil included); a micro-op map with other
    keys than the ones the columns hold; a :final? read that names an id twice (its raw vector and its map differ); a read whose
    sum of |credits| + |debits|, plus |total_amount|, reaches 2^63 (no device sum can wrap below that)."""

    def __init__(self, history, total_amount=0):
        total_amount = _i64(total_amount, "total-amount", -1)
        pos, type_, kind, flags, mop_n = [], [], [], [], []
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
        flush()
        self.total_amount = total_amount
        self.index = np.array(pos, np.uint32)
        self.type, self.kind, self.flags = np.array(type_, np.uint8), np.array(kind, np.uint8), np.array(flags, np.uint8)
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


def test(opts=None, linear=False, device_route=True):
    """The ledger test map (tests/ledger.clj:341-369) without generators: accounts, max-transfer, total-amount and the composed checker
    -- SI, lookup-transfers, final-reads, unexpected-ops, and with linear=True the member clj/patches/ledger.patch adds.
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
    if linear:
        members["linear"] = _Linear(opts["accounts"], bool(opts.get("negative-balances?", False)))
    return dict(opts, checker=jc.compose(members))

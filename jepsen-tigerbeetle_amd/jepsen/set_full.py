"""jepsen.checker/set-full on the MI355X -- the checker the reference runs for its set-full workload
(/root/reference/src/tigerbeetle/workloads/set_full.clj:155-158:
`(independent/checker (checker/compose {:set-full (checker/set-full {:linearizable? true}) ...}))`).

Host side: flatten the history into the reads x elements membership matrix and four index columns, call
`tbc_setfull_*` (csrc/set_full.hip scans the matrix for known / last-present / last-absent per element;
csrc/set_full_results.h decides every element's outcome and latencies and every key's counts, :valid?, latency
quantiles and worst stale elements from them, on the device), and name the elements in jepsen's result map
(:valid? :attempt-count :stable-count :lost :never-read :stale :worst-stale ...: `result_from_device`).  `result_map`
is the host statement of the same arithmetic from the three indices, kept for the tests to compare with.  The
semantics are recalled from jepsen.checker (jepsen is not in /root/reference and cannot run here) and
restated independently in oracle/set_full.py, which the tests compare with.  No CPU fallback: without a GPU
`check` raises NoDeviceError."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native as N
from ..columns import _p
from ..knossos import history as H

NONE = 0xFFFFFFFF


class Encoded:
    """reads x elements bit matrix + index columns of one history (one key).

    Recalled jepsen.checker/set-full details kept here: an :add INVOCATION creates the element's state, so adding an
    element again starts it afresh (its column is numbered by its LAST add invocation and only reads completing after
    that count); an element that occurs more than once in one read's value is a duplicate (`duplicated`: element ->
    greatest multiplicity seen), which makes the result invalid."""

    def __init__(self, history):
        hist = [op for op in H.index(list(history)) if H.client_op(op)]
        self.has_time = all("time" in op for op in hist) and bool(hist)
        self.times = {op["index"]: op.get("time", op["index"]) for op in hist}
        # the same as ONE column for the device (tbc_setfull_times.op_time: a slot per op of the history, client op or not), built once;
        # None when no op carries :time -- the library then takes the op index, as `times` does
        self.n_ops = (hist[-1]["index"] + 1) if hist else 0
        self.unit = 1_000_000 if self.has_time else 1
        self.op_time = None
        if any("time" in op for op in hist):
            self.op_time = np.zeros(self.n_ops, np.int64)
            self.op_time[[op["index"] for op in hist]] = [self.times[op["index"]] for op in hist]
        last_invoke, add_ok, reads, open_reads = {}, {}, [], {}
        self.duplicated = {}
        for op in hist:
            i = op["index"]
            if op["f"] == "add":
                v = _freeze(op["value"])
                if op["type"] == "invoke":
                    last_invoke[v] = (i, op["value"])
                    add_ok.pop(v, None)                        # a fresh element state: nothing known yet
                elif op["type"] == "ok" and v in last_invoke and v not in add_ok:
                    add_ok[v] = i
            elif op["f"] == "read":
                if op["type"] == "invoke":
                    open_reads[op["process"]] = i
                elif op["type"] == "fail":
                    open_reads.pop(op["process"], None)
                elif op["type"] == "ok":
                    inv = open_reads.pop(op["process"], None)
                    if inv is not None and op.get("value") is not None:
                        reads.append((inv, i, op["value"]))
        reads.sort(key=lambda r: r[0])
        by_invoke = sorted(last_invoke.items(), key=lambda kv: kv[1][0])
        order = [val for _, (_, val) in by_invoke]
        elems = {k: (n, inv) for n, (k, (inv, _)) in enumerate(by_invoke)}
        self.elements = order
        E, R = len(order), len(reads)
        self.E, self.R = E, R
        self.wpr = max(1, (E + 31) // 32)
        self.add_invoke = np.array([elems[_freeze(v)][1] for v in order], np.uint32)
        self.add_ok = np.array([add_ok.get(_freeze(v), NONE) for v in order], np.uint32)
        self.read_invoke = np.array([r[0] for r in reads], np.uint32)
        self.read_ok = np.array([r[1] for r in reads], np.uint32)
        # the reads in COMPACT form (tbc_setfull_rows): top[r] = every element numbered below it is in read r, except the listed
        # exceptions -- a listed element below top is absent, one at or above it present.  A read of a grow-only set is a prefix of
        # the elements in add-invocation order with a few holes, so top = greatest element read + 1 and the holes are the list.
        self.top = np.zeros(max(R, 1), np.uint32)
        self.exc_off = np.zeros(R + 1, np.uint64)
        exc_parts = []
        cols_of = []                                       # per read: the column numbers it contains (sorted, unique)
        ints = all(isinstance(v, int) and not isinstance(v, bool) for v in order)
        if ints and E:
            keys = np.array(order, np.int64)
            srt = np.argsort(keys)
            ks = keys[srt]
        for r, (_, _, val) in enumerate(reads):
            vals = list(val)
            if not vals:
                continue
            if ints and E and all(isinstance(x, int) and not isinstance(x, bool) for x in vals):
                arr = np.asarray(vals, np.int64)
                if len(arr) > 1:
                    u, c = np.unique(arr, return_counts=True)
                    for x, n in zip(u[c > 1].tolist(), c[c > 1].tolist()):
                        self.duplicated[x] = max(self.duplicated.get(x, 0), n)
                pos = np.minimum(np.searchsorted(ks, arr), E - 1)
                hit = ks[pos] == arr                       # values nobody added are not columns: jepsen ignores them here too
                cols_of.append((r, np.unique(srt[pos[hit]])))
            else:
                seen = {}
                for x in vals:
                    fx = _freeze(x)
                    seen[fx] = seen.get(fx, 0) + 1
                cols_of.append((r, np.unique(np.array([elems[fx][0] for fx in seen if fx in elems], np.int64))))
                for fx, n in seen.items():
                    if n > 1:
                        self.duplicated[fx] = max(self.duplicated.get(fx, 0), n)
        counts = np.zeros(R, np.int64)
        for r, cols in cols_of:
            if len(cols) == 0:
                continue
            t = int(cols[-1]) + 1
            self.top[r] = t
            holes = np.setdiff1d(np.arange(t, dtype=np.int64), cols, assume_unique=True)
            counts[r] = len(holes)
            if len(holes):
                exc_parts.append(holes.astype(np.uint32))
        self.exc_off[1:] = np.cumsum(counts)
        self.exc = np.concatenate(exc_parts) if exc_parts else np.zeros(0, np.uint32)
        self._cols_of = cols_of

    @property
    def present(self):
        """The dense reads x elements bit matrix (tbc_setfull_in.present), built on demand: the checker itself hands the compact form
        to the device, which builds the matrix there; tests and the dense entry point take this one."""
        bits = np.zeros((max(self.R, 1), self.wpr * 32), bool)
        for r, cols in self._cols_of:
            bits[r, cols] = True
        return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint32))


def _freeze(v):
    return tuple(v) if isinstance(v, list) else v


class _Handle:
    """A tbc_setfull / tbc_setfull_keys object: subclasses create `_h` and name the C calls; the handle's lifetime and the three result
    arrays of a run are the same for both."""
    _run = _destroy = _Out = None

    def _scan(self, n_elements):
        n = max(1, int(n_elements))
        known, lp, la = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        o = self._Out()
        o.known, o.last_present, o.last_absent = _p(known, C.c_uint32), _p(lp, C.c_uint32), _p(la, C.c_uint32)
        N.check_status(getattr(N.lib(), self._run)(self._h, C.byref(o)))
        return known, lp, la, {"ns_scan": o.ns_scan, "bytes_scanned": o.bytes_scanned, "bytes_matrix": o.bytes_matrix}

    def _decide(self, n_elements, n_keys, op_time, time_off, unit, linearizable, indices=False):
        """tbc_setfull_results / tbc_setfull_keys_results: -> per-element arrays over all keys, the per-key summaries (a ctypes array) and
        the call's totals.  op_time: one int64 array over all keys (time_off its n_keys + 1 offsets) or None (time = the op index)."""
        n = max(1, int(n_elements))
        outcome, slat, llat = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
        summary = (N.SetFullKeySummary * max(1, int(n_keys)))()
        t = N.SetFullTimes()
        keep = None
        if op_time is not None:
            keep = (np.ascontiguousarray(op_time if len(op_time) else np.zeros(1, np.int64), np.int64), np.ascontiguousarray(time_off, np.uint64))
            t.op_time, t.time_off = _p(keep[0], C.c_int64), _p(keep[1], C.c_uint64)
        t.unit, t.flags, t.reserved0 = int(unit), (N.SETFULL_F_LINEARIZABLE if linearizable else 0), 0
        o = N.SetFullResultsOut()
        o.outcome, o.stable_latency, o.lost_latency = _p(outcome, C.c_uint8), _p(slat, C.c_int64), _p(llat, C.c_int64)
        o.summary = summary
        arrays = {"outcome": outcome, "stable_latency": slat, "lost_latency": llat}
        if indices:
            for f in ("known", "last_present", "last_absent"):
                arrays[f] = np.zeros(n, np.uint32)
                setattr(o, f, _p(arrays[f], C.c_uint32))
        N.check_status(getattr(N.lib(), self._results)(self._h, C.byref(t), C.byref(o)))
        tot = {"ns_scan": o.ns_scan, "ns_results": o.ns_results, "bytes_scanned": o.bytes_scanned, "bytes_matrix": o.bytes_matrix}
        return arrays, summary, tot

    def close(self):
        if self._h:
            getattr(N.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Scan(_Handle):
    """tbc_setfull_*: the matrix resident in HBM, `run()` scans it."""
    _run, _destroy, _Out, _results = "tbc_setfull_run", "tbc_setfull_destroy", N.SetFullOut, "tbc_setfull_results"

    def __init__(self, enc_or_arrays, device=0, rows=None):
        """rows: True = hand the reads over in compact form (top / exc_off / exc: tbc_setfull_create_rows, the matrix is built on
        the device), False = the dense bit matrix (`present`); None = compact where the argument has it."""
        a = enc_or_arrays
        self._keep = a
        if rows is None:
            rows = hasattr(a, "top") and hasattr(a, "exc_off")
        self.E = a.E
        self._h = C.c_void_p()
        if rows:
            top = np.ascontiguousarray(a.top, np.uint32)
            off = np.ascontiguousarray(a.exc_off, np.uint64)
            exc = np.ascontiguousarray(a.exc if len(a.exc) else np.zeros(1, np.uint32), np.uint32)
            self._keep = (a, top, off, exc)
            s = N.SetFullRows()
            s.n_elements, s.n_reads, s.device, s.reserved0 = a.E, a.R, device, 0
            s.add_invoke, s.add_ok = _p(a.add_invoke, C.c_uint32), _p(a.add_ok, C.c_uint32)
            s.read_invoke, s.read_ok = _p(a.read_invoke, C.c_uint32), _p(a.read_ok, C.c_uint32)
            s.top, s.exc_off, s.exc = _p(top, C.c_uint32), _p(off, C.c_uint64), _p(exc, C.c_uint32)
            N.check_status(N.lib().tbc_setfull_create_rows(C.byref(s), C.byref(self._h)))
            return
        present = a.present
        self._keep = (a, present)
        s = N.SetFullIn()
        s.n_elements, s.n_reads, s.words_per_row, s.device = a.E, a.R, a.wpr, device
        s.add_invoke, s.add_ok = _p(a.add_invoke, C.c_uint32), _p(a.add_ok, C.c_uint32)
        s.read_invoke, s.read_ok = _p(a.read_invoke, C.c_uint32), _p(a.read_ok, C.c_uint32)
        s.present = _p(present, C.c_uint32)
        N.check_status(N.lib().tbc_setfull_create(C.byref(s), C.byref(self._h)))

    def run(self):
        known, lp, la, tot = self._scan(self.E)
        return {"known": known[:self.E], "last_present": lp[:self.E], "last_absent": la[:self.E], **tot}

    def results(self, times=None, unit=1, linearizable=False, indices=False):
        """The check result from the device (tbc_setfull_results): -> {"outcome", "stable_latency", "lost_latency" per element,
        "summary": the key's summary as a dict, "ns_scan", "ns_results", ...}.  times: the :time of every op of the history by op index
        (an int64 array, `Encoded.op_time`) or None = the op index; unit: what one latency unit is in those times (1,000,000: ns -> ms)."""
        off = None if times is None else np.array([0, len(times)], np.uint64)
        arrays, summary, tot = self._decide(self.E, 1, times, off, unit, linearizable, indices)
        return {**{f: a[:self.E] for f, a in arrays.items()}, "summary": summary_dict(summary[0]), **tot}


def frequency_distribution(points, xs):
    """jepsen.checker's latency summary (recalled): {point: the value at floor(n * point) of the sorted sample, clamped}."""
    srt = sorted(xs)
    n = len(srt)
    return {p: srt[min(n - 1, int(n * p))] for p in points} if n else None


def result_map(enc: Encoded, st: dict, linearizable: bool):
    """jepsen.checker/set-full's result from the three indices per element (vectorised: a few operations each).
    Latencies as jepsen computes them: max(0, dt) in nanoseconds -> whole milliseconds (util/nanos->ms, then long)
    when the ops carry :time; histories without :time (hand-written ones) keep the index difference.  So a gap
    below one millisecond is not a stale read, exactly as in jepsen."""
    k = st["known"].astype(np.int64)
    lp = np.where(st["last_present"] == NONE, -1, st["last_present"].astype(np.int64))
    la = np.where(st["last_absent"] == NONE, -1, st["last_absent"].astype(np.int64))
    known = st["known"] != NONE
    stable = (lp >= 0) & (la < lp)
    lost = known & (la >= 0) & (lp < la) & (k < la)
    never = ~(stable | lost)
    t = enc.times
    tk = np.array([t[int(x)] if kn else 0 for x, kn in zip(k, known)], np.int64)
    t_la = np.array([t[int(x)] + 1 if x >= 0 else 0 for x in la], np.int64)
    t_lp = np.array([t[int(x)] + 1 if x >= 0 else 0 for x in lp], np.int64)
    unit = 1_000_000 if getattr(enc, "has_time", False) else 1
    stable_lat = np.maximum(0, t_la - tk) // unit
    lost_lat = np.maximum(0, t_lp - tk) // unit
    el = enc.elements
    idx = lambda m: [el[i] for i in np.nonzero(m)[0]]
    stale = stable & (stable_lat > 0)
    worst = sorted(np.nonzero(stale)[0], key=lambda i: -int(stable_lat[i]))[:8]
    dups = dict(sorted(getattr(enc, "duplicated", {}).items(), key=lambda kv: repr(kv[0])))
    valid = False if lost.any() else ("unknown" if not stable.any() else (False if (linearizable and stale.any()) else True))
    if dups:
        valid = False                                   # (and (empty? dups) (:valid? results)): nil / :unknown -> falsey
    points = (0, 0.5, 0.95, 0.99, 1)
    out = {"valid?": valid, "attempt-count": enc.E, "stable-count": int(stable.sum()), "lost-count": int(lost.sum()),
           "lost": _sorted(idx(lost)), "never-read-count": int(never.sum()), "never-read": _sorted(idx(never)),
           "stale-count": int(stale.sum()), "stale": _sorted(idx(stale)),
           "worst-stale": [{"element": el[i], "outcome": "stable", "stable-latency": int(stable_lat[i]), "lost-latency": None,
                            "known": int(k[i]), "last-absent": int(la[i]) if la[i] >= 0 else None} for i in worst],
           "duplicated-count": len(dups), "duplicated": dups}
    if stable.any():
        out["stable-latencies"] = frequency_distribution(points, [int(x) for x in stable_lat[stable]])
    if lost.any():
        out["lost-latencies"] = frequency_distribution(points, [int(x) for x in lost_lat[lost]])
    return out


def _sorted(xs):
    try:
        return sorted(xs)
    except TypeError:
        return xs


QUANTILE_POINTS = (0, 0.5, 0.95, 0.99, 1)
_VALID = {N.SETFULL_VALID_FALSE: False, N.SETFULL_VALID_TRUE: True, N.SETFULL_VALID_UNKNOWN: "unknown"}


def summary_dict(s):
    """A tbc_setfull_key_summary as plain Python values."""
    nw = int(s.n_worst)
    none = lambda x: None if x == NONE else int(x)
    return {"attempt_count": int(s.attempt_count), "stable_count": int(s.stable_count), "lost_count": int(s.lost_count),
            "never_read_count": int(s.never_read_count), "stale_count": int(s.stale_count), "valid": _VALID[int(s.valid)],
            "stable_q": list(s.stable_q) if s.stable_q_present else None, "lost_q": list(s.lost_q) if s.lost_q_present else None,
            "worst": [{"element": int(s.worst_element[i]), "latency": int(s.worst_latency[i]), "known": none(s.worst_known[i]),
                       "last_absent": none(s.worst_last_absent[i])} for i in range(nw)]}


def result_from_device(enc: Encoded, dev: dict):
    """jepsen.checker/set-full's result map from what the device decided (`Scan.results` / `KeyedScan.results`: the outcome byte and
    the stable latency per element, the key's summary): nothing is computed here but WHICH elements the lists name -- np.nonzero over
    the outcome bytes -- and the one thing the device cannot know, the encoder's duplicates, which make any verdict false."""
    oc, s, el = dev["outcome"], dev["summary"], enc.elements
    names = lambda mask: _sorted([el[i] for i in np.nonzero(mask)[0].tolist()])
    dups = dict(sorted(getattr(enc, "duplicated", {}).items(), key=lambda kv: repr(kv[0])))
    out = {"valid?": False if dups else s["valid"],     # (and (empty? dups) (:valid? results)): nil / :unknown -> falsey
           "attempt-count": s["attempt_count"], "stable-count": s["stable_count"], "lost-count": s["lost_count"],
           "lost": names(oc == N.SETFULL_LOST), "never-read-count": s["never_read_count"], "never-read": names(oc == N.SETFULL_NEVER_READ),
           "stale-count": s["stale_count"], "stale": names((oc == N.SETFULL_STABLE) & (dev["stable_latency"] > 0)),
           "worst-stale": [{"element": el[w["element"]], "outcome": "stable", "stable-latency": w["latency"], "lost-latency": None,
                            "known": w["known"], "last-absent": w["last_absent"]} for w in s["worst"]],
           "duplicated-count": len(dups), "duplicated": dups}
    if s["stable_q"] is not None:
        out["stable-latencies"] = dict(zip(QUANTILE_POINTS, s["stable_q"]))
    if s["lost_q"] is not None:
        out["lost-latencies"] = dict(zip(QUANTILE_POINTS, s["lost_q"]))
    return out


def check(history, linearizable=False, device=0):
    enc = Encoded(history)
    with Scan(enc, device) as s:
        dev = s.results(enc.op_time, enc.unit, linearizable)
    return result_from_device(enc, dev)


# ---------------------------------------------------------------------------------------------------- many keys, one device pass
# The matrix bytes one keyed object may hold (the sum over its keys of reads x padded row): check_keys splits a larger independent
# history into several calls of at most this much each, one key never split.  (Tests lower it to force the split.)
KEYS_BUDGET_BYTES = 2 << 30


def _matrix_bytes(enc):
    return int(enc.R) * ((int(enc.wpr) + 3) // 4 * 4) * 4 if enc.E else 0


class KeyedScan(_Handle):
    """tbc_setfull_keys_*: the compact reads of MANY keys (each an `Encoded`) resident in one object; `run()` scans all of them in one
    fixed sequence of launches and returns each key's known / last-present / last-absent, in the order the encodings were given."""
    _run, _destroy, _Out, _results = "tbc_setfull_keys_run", "tbc_setfull_keys_destroy", N.SetFullKeysOut, "tbc_setfull_keys_results"

    def __init__(self, encs, device=0):
        encs = list(encs)
        self.Es = np.array([e.E for e in encs], np.uint32)
        self.Rs = np.array([e.R for e in encs], np.uint32)
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt) for x in parts] + [np.zeros(0, dt)]), dt)
        n_exc = [int(e.exc_off[e.R]) for e in encs]
        base = np.concatenate([[0], np.cumsum(n_exc, dtype=np.int64)]).astype(np.uint64)
        a = dict(add_invoke=cat([e.add_invoke for e in encs], np.uint32), add_ok=cat([e.add_ok for e in encs], np.uint32),
                 read_invoke=cat([e.read_invoke for e in encs], np.uint32), read_ok=cat([e.read_ok for e in encs], np.uint32),
                 top=cat([e.top[:e.R] for e in encs], np.uint32),
                 exc_off=cat([np.zeros(1, np.uint64)] + [np.asarray(e.exc_off[1:e.R + 1], np.uint64) + b for e, b in zip(encs, base)], np.uint64),
                 exc=cat([e.exc[:n] for e, n in zip(encs, n_exc)], np.uint32))
        self._keep = a = {k: (v if len(v) else np.zeros(1, v.dtype)) for k, v in a.items()}      # (a valid pointer for every array)
        s = N.SetFullKeysIn()
        s.n_keys, s.device = len(encs), device
        s.n_elements, s.n_reads = _p(self.Es, C.c_uint32), _p(self.Rs, C.c_uint32)
        for f in ("add_invoke", "add_ok", "read_invoke", "read_ok", "top", "exc"):
            setattr(s, f, _p(a[f], C.c_uint32))
        s.exc_off = _p(a["exc_off"], C.c_uint64)
        self._h = C.c_void_p()
        N.check_status(N.lib().tbc_setfull_keys_create(C.byref(s), C.byref(self._h)))

    @classmethod
    def from_ops(cls, columns, device=0):
        """tbc_setfull_keys_create_ops: the keys of an `OpColumns` resident in one object, ENCODED BY THE LIBRARY (the host plans which
        value is which column and which :ok read is which row; the device looks every read value up and builds the matrix).  The object
        is an ordinary keyed one: `run()` and `results()` as ever, `encoding()` says what the library made of the ops."""
        c = columns
        self = cls.__new__(cls)
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)                     # (a valid pointer for every array)
        self._keep = k = {f: pad(getattr(c, f)) for f in ("op_off", "index", "type", "f", "process", "value", "val_off", "vals")}
        s = N.SetFullOpsIn()
        s.n_keys, s.device = len(c.keys), device
        s.op_off, s.val_off = _p(k["op_off"], C.c_uint64), _p(k["val_off"], C.c_uint64)
        s.index, s.type, s.f = _p(k["index"], C.c_uint32), _p(k["type"], C.c_uint8), _p(k["f"], C.c_uint8)
        s.process, s.value, s.vals = _p(k["process"], C.c_int64), _p(k["value"], C.c_int64), _p(k["vals"], C.c_int64)
        self._h = C.c_void_p()
        N.check_status(N.lib().tbc_setfull_keys_create_ops(C.byref(s), C.byref(self._h)))
        self.Es, self.Rs = np.zeros(len(c.keys), np.uint32), np.zeros(len(c.keys), np.uint32)
        e = N.SetFullEncoding()
        e.n_elements, e.n_reads = _p(self.Es, C.c_uint32), _p(self.Rs, C.c_uint32)
        N.check_status(N.lib().tbc_setfull_keys_encoding(self._h, C.byref(e)))
        return self

    def shape(self):
        """tbc_setfull_keys_shape: (sum of the keys' elements, sum of their reads)."""
        se, sr = C.c_uint64(), C.c_uint64()
        N.check_status(N.lib().tbc_setfull_keys_shape(self._h, C.byref(se), C.byref(sr)))
        return se.value, sr.value

    def encoding(self):
        """tbc_setfull_keys_encoding (an object made by `from_ops` only): -> {"n_elements", "n_reads", "dup_count", "unknown_values" per
        key; "element", "add_invoke", "add_ok", "dup_max" per element and "read_invoke", "read_ok" per read, key after key; "ns_encode"}."""
        sumE, sumR = self.shape()
        n = len(self.Es)
        out = {"n_elements": np.zeros(n, np.uint32), "n_reads": np.zeros(n, np.uint32), "element": np.zeros(sumE, np.int64),
               "add_invoke": np.zeros(sumE, np.uint32), "add_ok": np.zeros(sumE, np.uint32), "read_invoke": np.zeros(sumR, np.uint32),
               "read_ok": np.zeros(sumR, np.uint32), "dup_max": np.zeros(sumE, np.uint32), "dup_count": np.zeros(n, np.uint32),
               "unknown_values": np.zeros(n, np.uint64)}
        e = N.SetFullEncoding()
        for f, a in out.items():
            if len(a):
                setattr(e, f, _p(a, {np.dtype(np.uint32): C.c_uint32, np.dtype(np.int64): C.c_int64, np.dtype(np.uint64): C.c_uint64}[a.dtype]))
        N.check_status(N.lib().tbc_setfull_keys_encoding(self._h, C.byref(e)))
        out["ns_encode"] = int(e.ns_encode)
        return out

    def run(self):
        """-> ([per key {"known", "last_present", "last_absent"}], {"ns_scan", "bytes_scanned", "bytes_matrix"} of the whole object)"""
        known, lp, la, tot = self._scan(self.Es.sum())
        cut = np.concatenate([[0], np.cumsum(self.Es, dtype=np.int64)])
        per = [{"known": known[a:b], "last_present": lp[a:b], "last_absent": la[a:b]} for a, b in zip(cut[:-1], cut[1:])]
        return per, tot

    def results(self, times=None, unit=1, linearizable=False, indices=False):
        """tbc_setfull_keys_results: -> ([per key what `Scan.results` gives without the totals], the totals of the whole object).
        times: per key an int64 array (the :time of every op of the key's history by op index), or None = the op index for every key."""
        op_time = off = None
        if times is not None:
            times = [np.asarray(t, np.int64) for t in times]
            off = np.concatenate([[0], np.cumsum([len(t) for t in times], dtype=np.int64)]).astype(np.uint64)
            op_time = np.concatenate(times + [np.zeros(0, np.int64)])
        arrays, summary, tot = self._decide(self.Es.sum(), len(self.Es), op_time, off, unit, linearizable, indices)
        cut = np.concatenate([[0], np.cumsum(self.Es, dtype=np.int64)])
        per = [{**{f: x[a:b] for f, x in arrays.items()}, "summary": summary_dict(summary[k])} for k, (a, b) in enumerate(zip(cut[:-1], cut[1:]))]
        return per, tot


def groups_within_budget(encs, budget=None):
    """The keys (a list of (key, Encoded)) in order, cut into runs of at most `budget` matrix bytes each (a larger key alone)."""
    budget = KEYS_BUDGET_BYTES if budget is None else budget
    out, cur, size = [], [], 0
    for k, e in encs:
        b = _matrix_bytes(e)
        if cur and size + b > budget:
            out.append(cur)
            cur, size = [], 0
        cur.append((k, e))
        size += b
    if cur:
        out.append(cur)
    return out


def scan_keys(encs, device=0):
    """{k: Encoded} -> {k: the three indices per element}: one keyed object per budget group (csrc/set_full.hip tbc_setfull_keys_*)."""
    out = {}
    for grp in groups_within_budget(list(encs.items())):
        with KeyedScan([e for _, e in grp], device) as ks:
            per, _ = ks.run()
        out.update({k: st for (k, _), st in zip(grp, per)})
    return out


def _time_column(enc):
    return enc.op_time if enc.op_time is not None else np.arange(enc.n_ops, dtype=np.int64)


def results_keys(encs, linearizable=False, device=0):
    """{k: Encoded} -> {k: what the device decided for the key (`KeyedScan.results`)}: one keyed object, one scan and one deciding pass
    per budget group.  A call has ONE latency unit: keys whose ops all carry :time (ns -> ms) and keys that lack some go in calls of
    their own."""
    out = {}
    for unit in sorted({e.unit for e in encs.values()}):
        part = [(k, e) for k, e in encs.items() if e.unit == unit]
        for grp in groups_within_budget(part):
            times = None if all(e.op_time is None for _, e in grp) else [_time_column(e) for _, e in grp]
            with KeyedScan([e for _, e in grp], device) as ks:
                per, _ = ks.results(times, unit, linearizable)
            out.update({k: dev for (k, _), dev in zip(grp, per)})
    return {k: out[k] for k in encs}


def check_keys(histories, linearizable=False, device=0):
    """{k: history} -> {k: set-full result}: each key encoded as `check` encodes it, all keys scanned and decided in one device pass
    per budget group; per key exactly what `check(history, linearizable)` gives."""
    if not histories:
        return {}
    encs = {k: Encoded(h) for k, h in histories.items()}
    devs = results_keys(encs, linearizable, device)
    return {k: result_from_device(encs[k], devs[k]) for k in encs}


# ---------------------------------------------------------------------------------------------------- the history as op columns
_TYPE_CODE = {"invoke": N.SETFULL_T_INVOKE, "ok": N.SETFULL_T_OK, "fail": N.SETFULL_T_FAIL, "info": N.SETFULL_T_INFO}
_F_CODE = {"add": N.SETFULL_OP_ADD, "read": N.SETFULL_OP_READ}
_I64 = (-(2 ** 63), 2 ** 63)


class OpColumns:
    """The client ops of one history (`OpColumns(history)`) or of the keys of an independent one (`OpColumns.of_keys({k: history})`) as
    the flat columns of tbc_setfull_ops_in: index, type, f, process, value per op, and the :ok reads' values end to end.  One plain pass
    that copies; it knows none of set-full's rules (the library applies them: `KeyedScan.from_ops`).  An element or a read value that
    is not an int in int64 range raises ValueError (such histories keep `Encoded`).  Per key it also keeps what `Encoded` keeps about
    time: `op_time` (a slot per op of the key's history, None if no op carries :time), `unit`, `n_ops`."""

    def __init__(self, history):
        self._fill({0: history})

    @classmethod
    def of_keys(cls, histories):
        self = cls.__new__(cls)
        self._fill(histories)
        return self

    def _fill(self, histories):
        self.keys = list(histories)
        index, type_, f_, process, value, val_n, parts = [], [], [], [], [], [], []
        op_off = [0]
        self.op_time, self.unit, self.n_ops, self.n_add_invokes, self.n_ok_reads = [], [], [], [], []
        for k, history in histories.items():
            n_time = n_client = n_inv = n_ok = 0
            last = -1
            times = []
            for i, op in enumerate(history):
                if not H.client_op(op):
                    continue
                n_client += 1
                last = i
                if "time" in op:
                    n_time += 1
                    times.append((i, op["time"]))
                t, f = _TYPE_CODE.get(op.get("type")), _F_CODE.get(op.get("f"), N.SETFULL_OP_OTHER)
                if t is None:
                    t, f = N.SETFULL_T_INFO, N.SETFULL_OP_OTHER
                v, nv = 0, 0
                if f == N.SETFULL_OP_ADD:
                    v = op.get("value")
                    if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or not _I64[0] <= v < _I64[1]:
                        raise ValueError(f"key {k!r} op {i}: the element {v!r} is not an int in int64 range (use Encoded)")
                    v = int(v)
                    n_inv += t == N.SETFULL_T_INVOKE
                elif f == N.SETFULL_OP_READ and t == N.SETFULL_T_OK:
                    rv = op.get("value")
                    if rv is None:
                        t |= N.SETFULL_T_NIL
                    else:
                        n_ok += 1
                        try:
                            arr = np.asarray(rv if isinstance(rv, (list, tuple, np.ndarray)) else list(rv))
                        except OverflowError:
                            arr = np.zeros(1, object)
                        if arr.size and (arr.ndim != 1 or arr.dtype.kind not in "iu" or (arr.dtype.kind == "u" and arr.size and int(arr.max()) >= _I64[1])):
                            raise ValueError(f"key {k!r} op {i}: a read value is not an int in int64 range (use Encoded)")
                        nv = int(arr.size)
                        if nv:
                            parts.append(arr.astype(np.int64, copy=False))
                index.append(i); type_.append(t); f_.append(f); process.append(op["process"]); value.append(v); val_n.append(nv)
            op_off.append(len(index))
            n_ops = last + 1
            self.n_ops.append(n_ops)
            self.unit.append(1_000_000 if n_client and n_time == n_client else 1)
            self.n_add_invokes.append(int(n_inv)); self.n_ok_reads.append(n_ok)
            col = None
            if n_time:                                   # as Encoded: an op without :time counts as its index
                col = np.zeros(n_ops, np.int64)
                if n_time != n_client:
                    col[index[op_off[-2]:]] = index[op_off[-2]:]
                col[[i for i, _ in times]] = [t for _, t in times]
            self.op_time.append(col)
        try:
            self.process = np.array(process, np.int64).reshape(-1)
        except OverflowError:
            raise ValueError("a process number is not in int64 range") from None
        self.op_off = np.array(op_off, np.uint64)
        self.index, self.type, self.f = np.array(index, np.uint32), np.array(type_, np.uint8), np.array(f_, np.uint8)
        self.value = np.array(value, np.int64).reshape(-1)
        self.val_off = np.concatenate([[0], np.cumsum(np.array(val_n, np.int64))]).astype(np.uint64)
        self.vals = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.int64)

    def take(self, positions):
        """The columns of the keys at `positions` (in that order) as an OpColumns of their own."""
        positions = list(positions)
        if positions == list(range(len(self.keys))):
            return self
        c = OpColumns.__new__(OpColumns)
        c.keys = [self.keys[p] for p in positions]
        for f in ("op_time", "unit", "n_ops", "n_add_invokes", "n_ok_reads"):
            setattr(c, f, [getattr(self, f)[p] for p in positions])
        lo, hi = self.op_off[positions].astype(np.int64), self.op_off[[p + 1 for p in positions]].astype(np.int64)
        rows = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
        for f in ("index", "type", "f", "process", "value"):
            setattr(c, f, np.ascontiguousarray(getattr(self, f)[rows]))
        c.op_off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint64)
        vo = self.val_off.astype(np.int64)
        c.val_off = np.concatenate([[0], np.cumsum(vo[rows + 1] - vo[rows])]).astype(np.uint64)
        c.vals = np.ascontiguousarray(np.concatenate([self.vals[vo[a]:vo[b]] for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]))
        return c


class _Named:
    """What `result_from_device` asks of an encoding: the elements' names and the duplicates."""

    def __init__(self, elements, duplicated):
        self.elements, self.duplicated = elements, duplicated


class _Bound:
    """The matrix a key of the columns can make at most: (:ok reads) x (add invocations)."""

    def __init__(self, n_add_invokes, n_ok_reads):
        self.E, self.R, self.wpr = n_add_invokes, n_ok_reads, max(1, (n_add_invokes + 31) // 32)


def unknown_duplicates(cols, k, elements, read_ok):
    """jepsen's `frequencies` over the whole read for the values the library does not see: {value: its greatest multiplicity within
    one read} over the values of key k's reads (`read_ok`: their :ok ops) that name none of `elements`.  One vectorised pass."""
    o0, o1 = int(cols.op_off[k]), int(cols.op_off[k + 1])
    rows = o0 + np.searchsorted(cols.index[o0:o1], read_ok)
    vo = cols.val_off.astype(np.int64)
    starts, lens = vo[rows], vo[rows + 1] - vo[rows]
    total = int(lens.sum())
    if total < 2:
        return {}
    at = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total)
    v, rid = cols.vals[at], np.repeat(np.arange(len(rows)), lens)
    m = ~np.isin(v, elements)
    v, rid = v[m], rid[m]
    if len(v) < 2:
        return {}
    order = np.lexsort((v, rid))
    v, rid = v[order], rid[order]
    first = np.concatenate([[True], (v[1:] != v[:-1]) | (rid[1:] != rid[:-1])])
    counts = np.diff(np.concatenate([np.nonzero(first)[0], [len(v)]]))
    vv = v[first]
    u, inv = np.unique(vv[counts > 1], return_inverse=True)
    mx = np.zeros(len(u), np.int64)
    np.maximum.at(mx, inv, counts[counts > 1])
    return dict(zip(u.tolist(), mx.tolist()))


def duplicated_of_key(cols, k, element, dup_max, unknown_values, read_ok):
    """jepsen's `duplicated` of key k of `cols` from the library's encoding of it (tbc_setfull_encoding, the key's slices): the elements
    with dup_max > 1, and -- only if the key has unknown values at all -- the duplicates among those."""
    dups = dict(zip(element[dup_max > 1].tolist(), dup_max[dup_max > 1].tolist()))
    if unknown_values:
        dups.update(unknown_duplicates(cols, k, element, read_ok))
    return dups


def check_keys_columns(histories, linearizable=False, device=0):
    """{k: history} -> {k: set-full result}, exactly what `check_keys` returns, with the ENCODING done by the library: the histories are
    copied into op columns (`OpColumns`), each budget group of keys becomes one object (`KeyedScan.from_ops`), and the result maps name
    their elements from the library's encoding.  `duplicated` comes from the library's dup_max; duplicates among values that name no
    element (which the library only counts) are added here, for the keys that have such values."""
    if not histories:
        return {}
    cols = OpColumns.of_keys(histories)
    out = {}
    for unit in sorted(set(cols.unit)):
        part = [(p, _Bound(cols.n_add_invokes[p], cols.n_ok_reads[p])) for p in range(len(cols.keys)) if cols.unit[p] == unit]
        for grp in groups_within_budget(part):
            pos = [p for p, _ in grp]
            sub = cols.take(pos)
            times = None if all(t is None for t in sub.op_time) else [t if t is not None else np.arange(n, dtype=np.int64)
                                                                        for t, n in zip(sub.op_time, sub.n_ops)]
            with KeyedScan.from_ops(sub, device) as ks:
                enc = ks.encoding()
                per, _ = ks.results(times, unit, linearizable)
            ce = np.concatenate([[0], np.cumsum(enc["n_elements"], dtype=np.int64)])
            cr = np.concatenate([[0], np.cumsum(enc["n_reads"], dtype=np.int64)])
            for j, p in enumerate(pos):
                el = enc["element"][ce[j]:ce[j + 1]]
                dm = enc["dup_max"][ce[j]:ce[j + 1]]
                dups = duplicated_of_key(sub, j, el, dm, enc["unknown_values"][j], enc["read_ok"][cr[j]:cr[j + 1]])
                out[cols.keys[p]] = result_from_device(_Named(el.tolist(), dups), per[j])
    return {k: out[k] for k in cols.keys}


def check_columns(history, linearizable=False, device=0):
    """`check` with the encoding done by the library (`check_keys_columns` of one key)."""
    return check_keys_columns({0: history}, linearizable, device)[0]


# ---------------------------------------------------------------------------------------------------- read-all-invoked-adds
def read_all_invoked_adds(history, enc=None):
    """The reference's `read-all-invoked-adds` (workloads/set_full.clj:51-75): did every :ok read with :final? see every value some
    :add was invoked with (crashed adds included)?  A nil value reads as empty; values read but never added do not count.
    -> {"valid?": True} or {"valid?": False, "suspect-final-reads": [[index, missing values sorted], ...]} in history order,
    index as the set-full result numbers ops (H.index over this history).

    With `enc` (this history's `Encoded`), a final read the encoding holds is answered from its compact row -- the missing values are
    the row's exceptions below top and the columns from top on that are not exceptions; any other final read (nil value, unmatched
    invoke) directly.  No device work either way."""
    hist = H.index(list(history))
    invoked = {}                                        # value -> (its last add invocation, the value): the encoding's column order
    for op in hist:
        if op.get("f") == "add" and op.get("type") == "invoke":
            invoked[_freeze(op.get("value"))] = (op["index"], op.get("value"))
    finals = [op for op in hist if op.get("f") == "read" and op.get("type") == "ok" and op.get("final?")]
    if not finals:
        return {"valid?": True}
    in_order = [v for _, v in sorted(invoked.values(), key=lambda iv: iv[0])]
    row_of = {}
    if enc is not None and len(enc.elements) == len(invoked) and all(_freeze(v) in invoked for v in enc.elements):
        row_of = {int(i): r for r, i in enumerate(enc.read_ok)}
    suspects = []
    for op in finals:
        r = row_of.get(op["index"])
        if r is not None:
            t = int(enc.top[r])
            exc = np.asarray(enc.exc[int(enc.exc_off[r]):int(enc.exc_off[r + 1])], np.int64)
            cols = np.union1d(exc[exc < t], np.setdiff1d(np.arange(t, enc.E, dtype=np.int64), exc))
            missing = [enc.elements[int(c)] for c in cols]
        else:
            seen = {_freeze(x) for x in (op.get("value") or [])}
            missing = [v for v in in_order if _freeze(v) not in seen]
        if missing:
            suspects.append([op["index"], _sorted(missing)])
    return {"valid?": False, "suspect-final-reads": suspects} if suspects else {"valid?": True}

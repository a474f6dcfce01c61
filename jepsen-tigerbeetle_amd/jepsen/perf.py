"""tigerbeetle.checker.perf -- the SERIES behind the reference's perf plots (checker/perf.clj, composed into every test as `perf`,
core.clj:139-146).  What the reference draws -- gnuplot, ranges, nemesis regions and lines, colours, PNG files (perf.clj:185-483) -- is
out of scope; what it draws them FROM is computed here:

* latency-raw        point-graph!      perf.clj:485-512   a point per invocation that has a completion
* latency-quantiles  quantiles-graph!  perf.clj:514-551   order statistics of the latencies per f and one-second bucket
* rate               rate-graph!       perf.clj:560-601   completions per f, type and bucket
* open-ops           open-ops-graph!   perf.clj:610-661   the running number of open ops per f and outcome

Two statements of the same series:

* the HOST statement, plain Python over op dicts written for clarity: `analyse` (everything as integers) and `series_host` (the four
  dicts).  It is the specification the device route is tested against.
* the DEVICE route: `PerfColumns` flattens the history into the columns of tbc_perf_in (include/tbcheck.h), `check_native` hands them
  to tbc_perf_series (csrc/perf_*.h) and `series_from_device` names the arrays that come back.  It has no host fallback: a history
  the columns cannot express raises ValueError, one the plan rejects TbcError, a missing device NoDeviceError.

The rules, in this library's words (ops are the dicts `edn.read_history` gives):

* CLIENT OP: `knossos.history.client_op` (perf.clj:570,620 filter on (integer? :process)).  Every other op -- the nemesis -- enters
  t_max and nothing else.
* PAIRING: `knossos.history.pair_index` as it stands (perf.clj:617 pair-index+): an invocation is completed by its process's next
  completion; a process that invokes again leaves its earlier invocation unmatched; a completion with nothing open pairs with nothing.
* OUTCOME of an op (perf.clj:623): for an invocation the type of its completion, None if it is unmatched; for a completion its OWN
  type.  This is knossos.history/completion as RECALLED (it gives an invocation's completion and a completion back unchanged); Knossos
  is not at hand, so the rule is unpinned.  `knossos/history.py::completion` gives the partner both ways and is not used here.
* LATENCY of a matched invocation (util/history->latencies, RECALLED): completion :time - invocation :time in ns, an integer; it may
  be negative where times are not monotone.  Milliseconds are ns / 1e6, formed on the host in both routes.  An UNMATCHED invocation
  has no latency: it is left out of the raw points and of the quantiles (the reference's latency-point would throw on its nil
  :latency, perf.clj:148-149).
* BUCKET of a time, dt = 1 s: t_ns // 10**9 on integers.  The reference computes long(double(t_ns) / 1e9) (util/nanos->secs, RECALLED:
  a division by 1e9; bucket-time, perf.clj:28-32) and the midpoint b + 1/2 (bucket-scale, :22-26); the two agree for
  0 <= t < 2**52 ns, and times outside that range, or ops without :time, are rejected.
* t_max = the largest :time of ALL ops, 0 at least (reduce max 0, perf.clj:566,616); nb_all = t_max // 10**9 + 1 buckets hold every op;
  n_plot = the buckets whose midpoint is <= t_max / 1e9 compared as doubles (buckets dt t-max, perf.clj:40-41) -- nb_all or
  nb_all - 1.  rate and open-ops are listed over the n_plot buckets only: what falls in an unplotted last bucket is not shown, as in
  the reference.
* latency_raw[(f, outcome)]: (t_s, ms) per matched invocation of f whose completion is `outcome`, in history order (:497-503).
* latency_quantiles[(f, q)], q in 0.5 0.95 0.99 1: per bucket of the INVOCATION's time that holds n >= 1 matched invocations of f, all
  outcomes together: (b + 0.5, sorted[min(n - 1, floor(n * q))]) with n * q in double (quantiles, :52-62; latencies->quantiles, :64-86).
* rate[(f, type)], type in ok info fail: for every plotted bucket count * 1.0 of the client completions of (f, type) whose own time is
  in it (:567-594); present only if (f, type) has a completion anywhere.  A completion without an invocation counts: it is a client
  op that is no invocation.
* open_ops[(f, outcome)]: a running count per (f, outcome) over the client ops that have an outcome, in history order: +1 at an
  invocation, -1 at a completion (:622-633).  Per (class, bucket of the op's own time) the value after the LAST such op in history
  order is kept; the series is its forward fill over the plotted buckets, from 0 (:644-654).  Present only if the class has an op.
  The count is >= 0 as long as every completion has its invocation (`analyse` asserts that); a completion WITHOUT one takes its own
  type's class below what was invoked, possibly below 0, exactly as the reference's reduce does.
* The f's of a series set are listed in util/polysort order (RECALLED: compare, and by class name where that throws), the types as
  ok info fail (perf.clj:175-177).

`perf(opts)` is the composed checker (perf.clj:700-708): its members latency-graph, rate-graph and open-ops-graph compute their
series and answer {"valid?": True} as the reference's do; no file is written and nothing is plotted.
"""
from __future__ import annotations

import ctypes as C
import functools
import threading

import numpy as np

from .. import _native as N
from ..knossos import history as H
from . import checker as jc

QS = (0.5, 0.95, 0.99, 1)
TYPES = ("ok", "info", "fail")                    # the order series are listed in
_TYPE = {"invoke": N.PERF_T_INVOKE, "ok": N.PERF_T_OK, "fail": N.PERF_T_FAIL, "info": N.PERF_T_INFO}
OUTCOMES = (None, "ok", "fail", "info")           # by TBC_PERF_T_* / TBC_PERF_O_NONE
SECOND = 10 ** 9
TIME_END = 2 ** 52
INT32_MIN, INT64_MIN = -(2 ** 31), -(2 ** 63)


def bucket(t_ns):
    """the one-second bucket of a time, on integers"""
    return t_ns // SECOND


def bucket_float(t_ns):
    """... as the reference computes it: long(double(t) / 1e9)"""
    return int(float(t_ns) / 1e9)


def plotted_buckets(t_max):
    """n_plot: how many of the midpoints 0.5, 1.5, ... are <= t_max / 1e9 (take-while over (buckets dt), perf.clj:40-41)"""
    nb_all = bucket(t_max) + 1
    return nb_all if (nb_all - 1) + 0.5 <= t_max / 1e9 else nb_all - 1


def rank(n, q):
    return min(n - 1, int(n * q))


def polysort(xs):
    """jepsen.util/polysort (RECALLED): sort by compare; values that do not compare, by the name of their class."""
    def cmp(a, b):
        try:
            return (a > b) - (a < b)
        except TypeError:
            ta, tb = type(a).__name__, type(b).__name__
            return (ta > tb) - (ta < tb)
    return sorted(xs, key=functools.cmp_to_key(cmp))


# ---------------------------------------------------------------- the host statement

def _time(op, i):
    t = op.get("time")
    if not isinstance(t, int) or isinstance(t, bool) or not 0 <= t < TIME_END:
        raise ValueError(f"op {i}: :time {t!r} is not an int in [0, 2^52) ns")
    return t


def analyse(history):
    """The host statement on integers.  A dict:
      fs            the f's of the client ops in order of first appearance
      t_max, nb_all, n_plot
      latency       per op: ns for a matched invocation, None otherwise
      outcome       per op: "ok" / "fail" / "info", None for an op without one (and for every op that is not a client's)
      open_after    per op: its class's running count after it; 0 for an op without an outcome
      q_cells       {f: {bucket: [latencies of the matched invocations whose own time is in it, ascending]}}
      rate          {(f, type): {bucket: completions}}
      open_last     {(f, outcome): {bucket: the count after the last op of the class in the bucket}}
    """
    pairs = H.pair_index(history)
    times = [_time(op, i) for i, op in enumerate(history)]
    t_max = max(times, default=0)
    fs, latency, outcome, open_after = [], [], [], []
    q_cells, rate, open_last, running = {}, {}, {}, {}
    orphans = False
    for i, op in enumerate(history):
        lat = out = None
        if H.client_op(op):
            if op["type"] not in _TYPE:
                raise ValueError(f"op {i}: type {op['type']!r}")
            f = op.get("f")
            if f not in fs:
                fs.append(f)
            if op["type"] == "invoke":
                j = pairs.get(i)
                if j is not None:
                    out, lat = history[j]["type"], times[j] - times[i]
                    q_cells.setdefault(f, {}).setdefault(bucket(times[i]), []).append(lat)
            else:
                out = op["type"]
                orphans = orphans or pairs.get(i) is None
                cell = rate.setdefault((f, out), {})
                cell[bucket(times[i])] = cell.get(bucket(times[i]), 0) + 1
        after = 0
        if out is not None:
            after = running.get((f, out), 0) + (1 if op["type"] == "invoke" else -1)
            assert after >= 0 or orphans, (i, after)        # the device keeps it in 32 bits either way
            running[(f, out)] = after
            open_last.setdefault((f, out), {})[bucket(times[i])] = after
        latency.append(lat); outcome.append(out); open_after.append(after)
    for cells in q_cells.values():
        for lats in cells.values():
            lats.sort()
    return {"fs": fs, "t_max": t_max, "nb_all": bucket(t_max) + 1, "n_plot": plotted_buckets(t_max), "latency": latency, "outcome": outcome,
            "open_after": open_after, "q_cells": q_cells, "rate": rate, "open_last": open_last}


def series_host(history):
    """The four series sets from the host statement."""
    a = analyse(history)
    fs, n_plot = polysort(a["fs"]), a["n_plot"]
    raw = {}
    for op, lat, out in zip(history, a["latency"], a["outcome"]):
        if lat is not None:
            raw.setdefault((op.get("f"), out), []).append((op["time"] / 1e9, lat / 1e6))
    latency_raw = {(f, t): raw[(f, t)] for f in fs for t in TYPES if (f, t) in raw}
    quantiles = {(f, q): [(b + 0.5, lats[rank(len(lats), q)] / 1e6) for b, lats in sorted(a["q_cells"][f].items())]
                 for f in fs if f in a["q_cells"] for q in QS}
    rate = {(f, t): [(b + 0.5, a["rate"][(f, t)].get(b, 0) * 1.0) for b in range(n_plot)] for f in fs for t in TYPES if (f, t) in a["rate"]}
    open_ops = {}
    for f in fs:
        for t in TYPES:
            if (f, t) not in a["open_last"]:
                continue
            cur, pts = 0, []
            for b in range(n_plot):
                cur = a["open_last"][(f, t)].get(b, cur)
                pts.append((b + 0.5, cur))
            open_ops[(f, t)] = pts
    return {"latency_raw": latency_raw, "latency_quantiles": quantiles, "rate": rate, "open_ops": open_ops}


# ---------------------------------------------------------------- the device route

class PerfColumns:
    """ALL ops of a history as the flat columns of tbc_perf_in, one row per op in history order: time (ns), process (INT32_MIN for an op
    that is not a client's), type, f (a number per distinct :f of the client ops, from 0 by first appearance; `fs` lists them) and flags
    (TBC_PERF_F_CLIENT).  One plain pass that copies; it applies no rule of the series.  An op without an integer :time is passed as
    INT64_MIN and a time out of range as it is: the plan rejects both (TBC_ERR_BAD_HISTORY).

    ValueError: a client op whose type is not invoke / ok / fail / info, whose :process is not in int32 range (INT32_MIN itself
    included), or more than 65536 distinct f's."""

    def __init__(self, history):
        n = len(history)
        self.time, self.process = np.zeros(n, np.int64), np.full(n, INT32_MIN, np.int32)
        self.type, self.flags, self.f = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
        ids = {}
        for i, op in enumerate(history):
            t = op.get("time")
            self.time[i] = t if isinstance(t, int) and not isinstance(t, bool) and INT64_MIN < t < -INT64_MIN else INT64_MIN
            if not H.client_op(op):
                self.type[i] = _TYPE.get(op.get("type"), N.PERF_T_INFO)
                continue
            if op.get("type") not in _TYPE:
                raise ValueError(f"op {i}: type {op.get('type')!r}")
            if not INT32_MIN < op["process"] < 2 ** 31:
                raise ValueError(f"op {i}: process {op['process']!r} is not in int32 range")
            f = ids.setdefault(op.get("f"), len(ids))
            if f >= 65536:
                raise ValueError(f"op {i}: more than 65536 distinct f's")
            self.process[i], self.type[i], self.flags[i], self.f[i] = op["process"], _TYPE[op["type"]], N.PERF_F_CLIENT, f
        self.fs = list(ids)

    def __len__(self):
        return len(self.time)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def perf_in(cols, device=0):
    """A tbc_perf_in over a PerfColumns (and the arrays it points into: keep them while the struct is used)."""
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    keep = {f: pad(np.ascontiguousarray(getattr(cols, f))) for f in ("time", "process", "type", "flags", "f")}
    s = N.PerfIn()
    s.n_ops, s.device, s.n_f = len(cols), device, len(cols.fs)
    s.time, s.process = _ptr(keep["time"], C.c_int64), _ptr(keep["process"], C.c_int32)
    s.type, s.flags, s.f = _ptr(keep["type"], C.c_uint8), _ptr(keep["flags"], C.c_uint8), _ptr(keep["f"], C.c_uint16)
    return s, keep


def plan_sizes(cols, call=None):
    """tbc_perf_plan_sizes: {"n_ops", "n_f", "nb_all", "n_plot", "t_max"} -- the host plan alone, no device.  call(in, sizes): another
    implementation (the tests' build of the same plan)."""
    s, keep = perf_in(cols)
    z = N.PerfSizes()
    if call is None:
        N.check_status(N.lib().tbc_perf_plan_sizes(C.byref(s), C.byref(z)))
    else:
        call(s, z)
    del keep
    return {f: int(getattr(z, f)) for f, _ in N.PerfSizes._fields_}


def summary_dict(s):
    return {f: int(getattr(s, f)) for f, _ in N.PerfSummary._fields_ if f != "reserved0"}


def check_native(cols, device=0, call=None, sizes_call=None):
    """tbc_perf_series over the columns -> the raw arrays, shaped as include/tbcheck.h gives them, and the summary (a dict).
    call(in, out) / sizes_call(in, sizes): other implementations of the two entry points (the tests' emulator build of the same kernels)."""
    z = plan_sizes(cols, sizes_call)
    n, nf, nb, npl = z["n_ops"], z["n_f"], z["nb_all"], z["n_plot"]
    shapes = {"op_latency": ((n,), np.int64), "op_outcome": ((n,), np.uint8), "op_open_after": ((n,), np.int32),
              "q_count": ((nf, nb), np.uint32), "q_value": ((nf, nb, 4), np.int64), "rate_count": ((nf, 3, nb), np.uint32),
              "open_last": ((nf, 3, nb), np.int32), "open_fill": ((nf, 3, npl), np.int32)}
    ct = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.int64): C.c_int64, np.dtype(np.uint32): C.c_uint32, np.dtype(np.int32): C.c_int32}
    arr = {f: np.zeros(max(1, int(np.prod(shape))), dt) for f, (shape, dt) in shapes.items()}
    s, keep = perf_in(cols, device)
    out = N.PerfOut()
    for f, x in arr.items():
        setattr(out, f, _ptr(x, ct[x.dtype]))
    if call is None:
        N.check_status(N.lib().tbc_perf_series(C.byref(s), C.byref(out)))
    else:
        call(s, out)
    del keep
    res = {f: arr[f][:int(np.prod(shape))].reshape(shape) for f, (shape, _) in shapes.items()}
    res["summary"] = summary_dict(out.summary)
    return res


def series_from_device(history, cols, dev):
    """The four series sets as `series_host` gives them, from tbc_perf_series' arrays: nothing is computed here but / 1e9, / 1e6, + 0.5
    and the names."""
    s = dev["summary"]
    nb_all, n_plot = s["nb_all"], s["n_plot"]
    num = {f: k for k, f in enumerate(cols.fs)}
    fs = polysort(cols.fs)
    raw = {}
    for i in np.flatnonzero(dev["op_latency"] != INT64_MIN):
        op = history[int(i)]
        raw.setdefault((op.get("f"), OUTCOMES[int(dev["op_outcome"][i])]), []).append((op["time"] / 1e9, int(dev["op_latency"][i]) / 1e6))
    latency_raw = {(f, t): raw[(f, t)] for f in fs for t in TYPES if (f, t) in raw}
    quantiles = {}
    for f in fs:
        cells = np.flatnonzero(dev["q_count"][num[f]])
        for j, q in enumerate(QS):
            if len(cells):
                quantiles[(f, q)] = [(int(b) + 0.5, int(dev["q_value"][num[f], b, j]) / 1e6) for b in cells]
    rate, open_ops = {}, {}
    for f in fs:
        for t in TYPES:
            o = _TYPE[t] - 1
            counts = dev["rate_count"][num[f], o]
            if counts.any():
                rate[(f, t)] = [(b + 0.5, int(counts[b]) * 1.0) for b in range(n_plot)]
            if (dev["open_last"][num[f], o] != INT32_MIN).any():
                open_ops[(f, t)] = [(b + 0.5, int(dev["open_fill"][num[f], o, b])) for b in range(n_plot)]
    assert dev["q_count"].shape[1] == nb_all
    return {"latency_raw": latency_raw, "latency_quantiles": quantiles, "rate": rate, "open_ops": open_ops}


def series_device(history, device=0):
    cols = PerfColumns(history)
    return series_from_device(history, cols, check_native(cols, device))


# The rule was set before measuring: the device route is the default only if the device call beats the host statement at 10^5 ops.  It
# does (profiles/NOTES_perf.md: 3 ms against 105-116 ms; with the columns pass and the naming of the series 78-208 ms against the
# 118-356 ms of `series_host`), so it is -- as ledger.test's is.  Without a gfx950 device the default raises NoDeviceError.
DEVICE_ROUTE_DEFAULT = True


def series(history, device_route=None, device=0):
    """{"latency_raw", "latency_quantiles", "rate", "open_ops"}: each a dict of (f, type) or (f, q) -> list of (x, y) points.
    device_route=True takes tbc_perf_series (no host fallback), False the host statement; None the measured default."""
    if DEVICE_ROUTE_DEFAULT if device_route is None else device_route:
        return series_device(history, device)
    return series_host(history)


class _Shared:
    """ONE `series` call per history for the three members of the compose (they run concurrently: the first to ask computes, the others
    wait for it); dropped when all three have had it."""

    def __init__(self, opts):
        self.opts, self.lock, self.key, self.res, self.left = dict(opts or {}), threading.Lock(), None, None, 0

    def result(self, history, opts):
        with self.lock:
            if self.key is not history:
                o = dict(self.opts)
                o.update(opts or {})
                self.key, self.res, self.left = None, None, 0
                self.res = series(history, o.get("device_route"), o.get("device", 0))
                self.key, self.left = history, 3
            res = self.res
            self.left -= 1
            if self.left == 0:
                self.key, self.res = None, None
            return res


class _Graph(jc.Checker):
    """A member of `perf`: the series are computed (so a history they cannot be made from raises, as the reference's plots throw) and
    the answer is {"valid?": True}."""

    def __init__(self, shared):
        self.shared = shared

    def check(self, test, history, opts=None):
        self.shared.result(history, opts)
        return {"valid?": True}


def perf(opts=None):
    """(perf opts), perf.clj:700-708: latency-graph (the raw points and the quantiles), rate-graph, open-ops-graph.  opts:
    "device_route" (None: the measured default), "device"."""
    shared = _Shared(opts)
    return jc.compose({"latency-graph": _Graph(shared), "rate-graph": _Graph(shared), "open-ops-graph": _Graph(shared)})

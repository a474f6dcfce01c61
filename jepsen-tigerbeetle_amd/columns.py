"""Column (SoA) forms of a history and the host-side pairing step.

`EventColumns` is one row per Jepsen op map (:type :process :f :value);
`OpColumns` is the history after knossos.history/complete + without-failures
+ pairing (tbc_pair_events in the library), which is what crosses the C-ABI.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N


def _p(arr, ct):
    return arr.ctypes.data_as(C.POINTER(ct))


@dataclass
class EventColumns:
    type: np.ndarray      # uint8
    process: np.ndarray   # int32
    f: np.ndarray         # uint8
    a: np.ndarray         # int32
    b: np.ndarray         # int32

    def __len__(self):
        return len(self.type)

    def struct(self) -> N.Events:
        e = N.Events()
        e.n = len(self.type)
        e.type = _p(self.type, C.c_uint8)
        e.process = _p(self.process, C.c_int32)
        e.f = _p(self.f, C.c_uint8)
        e.a = _p(self.a, C.c_int32)
        e.b = _p(self.b, C.c_int32)
        return e


@dataclass
class OpColumns:
    f: np.ndarray         # uint8
    a: np.ndarray         # int32
    b: np.ndarray         # int32
    process: np.ndarray   # int32, dense
    inv_pos: np.ndarray   # uint32, ascending
    ret_pos: np.ndarray   # uint32, POS_CRASHED for :info
    n_events: int
    n_process: int
    pool: np.ndarray = None   # int32 values of wide ops (multi-register micro-ops), or None

    def __len__(self):
        return len(self.f)

    def struct(self) -> N.Ops:
        o = N.Ops()
        o.n = len(self.f)
        o.n_events = self.n_events
        o.f = _p(self.f, C.c_uint8)
        o.a = _p(self.a, C.c_int32)
        o.b = _p(self.b, C.c_int32)
        o.process = _p(self.process, C.c_int32)
        o.inv_pos = _p(self.inv_pos, C.c_uint32)
        o.ret_pos = _p(self.ret_pos, C.c_uint32)
        if self.pool is not None and len(self.pool):
            o.pool = _p(self.pool, C.c_int32)
            o.pool_len = len(self.pool)
        else:
            o.pool = None
            o.pool_len = 0
        o.n_process = self.n_process
        return o

    def as_dict(self):
        return {"f": self.f, "a": self.a, "b": self.b, "process": self.process,
                "inv_pos": self.inv_pos, "ret_pos": self.ret_pos, "n_process": self.n_process, "pool": self.pool}


def pair_events(ev: EventColumns) -> OpColumns:
    """knossos.history/complete + without-failures + pairing (host code in the library)."""
    n = len(ev)
    f = np.zeros(max(n, 1), np.uint8)
    a = np.zeros(max(n, 1), np.int32)
    b = np.zeros(max(n, 1), np.int32)
    proc = np.zeros(max(n, 1), np.int32)
    inv = np.zeros(max(n, 1), np.uint32)
    ret = np.zeros(max(n, 1), np.uint32)
    n_ops = C.c_uint32(0)
    n_proc = C.c_uint32(0)
    es = ev.struct()
    st = N.lib().tbc_pair_events(C.byref(es), _p(f, C.c_uint8), _p(a, C.c_int32), _p(b, C.c_int32),
                                 _p(proc, C.c_int32), _p(inv, C.c_uint32), _p(ret, C.c_uint32),
                                 C.byref(n_ops), C.byref(n_proc))
    N.check_status(st)
    k = n_ops.value
    return OpColumns(f[:k].copy(), a[:k].copy(), b[:k].copy(), proc[:k].copy(), inv[:k].copy(), ret[:k].copy(),
                     n_events=n, n_process=n_proc.value)


def concat_events(evs):
    """Event histories side by side as tbc_event_batch takes them: (ev_off u64[n + 1], EventColumns of the concatenation)."""
    nh = len(evs)
    ev_off = np.zeros(nh + 1, np.uint64)
    if nh:
        np.cumsum(np.fromiter((len(e) for e in evs), np.uint64, nh), out=ev_off[1:])
    cat = lambda name, dt: (np.ascontiguousarray(np.concatenate([getattr(e, name) for e in evs]).astype(dt, copy=False))
                            if nh else np.zeros(0, dt))
    return ev_off, EventColumns(cat("type", np.uint8), cat("process", np.int32), cat("f", np.uint8), cat("a", np.int32), cat("b", np.int32))


def pack_events(ev: EventColumns, out=None) -> np.ndarray:
    """tbc_pack_events: one history's columns -> its packed event words (TBC_EVENT_WORD, uint32[len(ev)]); the process column
    travels beside them as it is.  out: where to write them (a view of a mapped event slot, core.Batch.map_events)."""
    n = len(ev)
    if out is None:
        out = np.zeros(n, np.uint32)
    elif len(out) != n or out.dtype != np.uint32 or not out.flags.c_contiguous:
        raise ValueError("pack_events: out must be a contiguous uint32 array of the history's length")
    es = ev.struct()
    N.check_status(N.lib().tbc_pack_events(C.byref(es), _p(out, C.c_uint32)))
    return out


def pair_events_batch_raw(ev_off, ev, ops_cap=None, columns=True, word=False, device=0, into=None, call=None, alloc=np.zeros):
    """tbc_pair_events_batch on concatenated event columns (concat_events) -- or tbc_pair_packed_batch, if `ev` is a pair
    (ev_word uint32[events], process int32[events]) of packed events.  -> (status of the call, dict of the output arrays
    and of n_bad, n_ops, ns_device, bytes_in).  ops_cap: the capacity of the op arrays (default: one op per event); columns: ask for
    f, a, b, process; word: ask for the wire word; into: a mapped input slot (core.Batch.map_input) whose op_off, n_events,
    n_process, word, inv_pos and ret_pos are written in place; call: another implementation of the entry point (the tests' emulator);
    alloc(n, dtype): where the op arrays come from (pinned memory, for a caller that has some)."""
    nh = len(ev_off) - 1
    n = int(ev_off[-1])
    cap = n if ops_cap is None else int(ops_cap)
    m = max(cap, 1)
    r = {"status": np.zeros(max(nh, 1), np.int32), "bad_row": np.zeros(max(nh, 1), np.uint32)}
    if into is None:
        r.update(op_off=np.zeros(nh + 1, np.uint64), n_events=np.zeros(max(nh, 1), np.uint32), n_process=np.zeros(max(nh, 1), np.uint32),
                 inv_pos=alloc(m, np.uint32), ret_pos=alloc(m, np.uint32))
        if word:
            r["word"] = alloc(m, np.uint32)
    else:
        if nh > into["n_hist_cap"]:
            raise ValueError(f"{nh} histories, the batch's slots hold {into['n_hist_cap']}")
        cap = int(into["ops_cap"]) if ops_cap is None else min(cap, int(into["ops_cap"]))
        r.update({k: into[k] for k in ("op_off", "n_events", "n_process", "inv_pos", "ret_pos", "word")})
    if columns:
        r.update(f=alloc(m, np.uint8), a=alloc(m, np.int32), b=alloc(m, np.int32), process=alloc(m, np.int32))
    packed = isinstance(ev, tuple)
    i = N.PackedEventBatch() if packed else N.EventBatch()
    i.n_hist, i.device, i.ev_off = nh, device, _p(ev_off, C.c_uint64)
    if packed:
        i.ev_word, i.process = _p(ev[0], C.c_uint32), _p(ev[1], C.c_int32)
    else:
        i.type, i.process, i.f, i.a, i.b = _p(ev.type, C.c_uint8), _p(ev.process, C.c_int32), _p(ev.f, C.c_uint8), _p(ev.a, C.c_int32), _p(ev.b, C.c_int32)
    o = N.PairOut()
    o.ops_cap = cap
    for name, ct in (("op_off", C.c_uint64), ("n_events", C.c_uint32), ("n_process", C.c_uint32), ("f", C.c_uint8), ("a", C.c_int32),
                     ("b", C.c_int32), ("process", C.c_int32), ("inv_pos", C.c_uint32), ("ret_pos", C.c_uint32), ("word", C.c_uint32),
                     ("status", C.c_int32), ("bad_row", C.c_uint32)):
        if name in r:
            setattr(o, name, _p(r[name], ct))
    st = (call or (N.lib().tbc_pair_packed_batch if packed else N.lib().tbc_pair_events_batch))(C.byref(i), C.byref(o))
    r.update(n_bad=int(o.n_bad), n_ops=int(o.n_ops), ns_device=int(o.ns_device), bytes_in=int(o.bytes_in))
    r["status"], r["bad_row"] = r["status"][:nh], r["bad_row"][:nh]
    return st, r


def pair_events_batch(evs, device=0):
    """tbc_pair_events_batch: pair_events for many histories in one call, on the device.
    -> (list of OpColumns, None where the history is refused; status int32[n]; bad_row uint32[n], PAIR_NO_ROW where there is none)."""
    ev_off, ev = concat_events(evs)
    st, r = pair_events_batch_raw(ev_off, ev, device=device)
    N.check_status(st)
    ops = []
    for h in range(len(evs)):
        if r["status"][h] != N.OK_STATUS:
            ops.append(None)
            continue
        lo, hi = int(r["op_off"][h]), int(r["op_off"][h + 1])
        ops.append(OpColumns(*[r[k][lo:hi].copy() for k in ("f", "a", "b", "process", "inv_pos", "ret_pos")],
                             n_events=int(r["n_events"][h]), n_process=int(r["n_process"][h])))
    return ops, r["status"], r["bad_row"]


def split_events(ev, key):
    """ONE event history whose rows belong to keys (jepsen.independent: values are [k v] tuples) split by key, in numpy -- THE
    DEFINITION of what tbc_pair_keyed_events splits on the device, and jepsen/independent.split restricted to tuple rows.
    `ev`: anything with a length (only len(ev) is looked at); key: int32[len(ev)], one key per row (rows that belong to every key --
    nemesis ops, non-tuple values -- are no client op of any key's object: the caller leaves them out).
    -> (keys int32[n_keys] in order of FIRST APPEARANCE, ev_off uint64[n_keys + 1], row_of uint32[n]): key k's rows are
    row_of[ev_off[k]:ev_off[k + 1]], in the order they had (a stable split)."""
    key = np.ascontiguousarray(key, np.int32)
    n = len(key)
    if len(ev) != n:
        raise ValueError(f"split_events: {len(ev)} rows, {n} keys")
    uniq, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                     # the distinct keys by their first row
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    ev_off = np.zeros(len(uniq) + 1, np.uint64)
    np.cumsum(counts[order], out=ev_off[1:])
    row_of = np.argsort(rank[inverse.reshape(-1)], kind="stable").astype(np.uint32)
    return uniq[order].astype(np.int32), ev_off, row_of


def take_events(ev: EventColumns, rows) -> EventColumns:
    """the rows `rows` of an event history, in that order"""
    return EventColumns(*[np.ascontiguousarray(getattr(ev, k)[rows]) for k in ("type", "process", "f", "a", "b")])


def pair_keyed_events_raw(ev, key, keys_cap=None, ops_cap=None, columns=True, word=False, row_of=True, pair=True, device=0, call=None):
    """tbc_pair_keyed_events: ONE keyed event history -- `ev` an EventColumns, or a pair (ev_word uint32[n], process int32[n]) of packed
    events (pack_events) -- split by key and paired per key on the device in one call.
    -> (status of the call, dict): keys, ev_off, row_of (split_events' three, the first n_keys / n_keys + 1 entries), n_keys, and -- with
    `pair` -- what pair_events_batch_raw returns over the keys' histories.  keys_cap: the keys the outputs hold (default: one per
    row); ops_cap, columns, word: as pair_events_batch_raw; row_of=False: not asked for; pair=False: split only (out = NULL);
    call: another implementation of the entry point (the tests' emulator)."""
    key = np.ascontiguousarray(key, np.int32)
    n = len(key)
    packed = isinstance(ev, tuple)
    if (len(ev[0]) if packed else len(ev)) != n:
        raise ValueError("pair_keyed_events_raw: one key per row")
    kc = n if keys_cap is None else int(keys_cap)
    cap = n if ops_cap is None else int(ops_cap)
    m = max(cap, 1)
    r = {"keys": np.zeros(max(kc, 1), np.int32), "ev_off": np.zeros(kc + 1, np.uint64)}
    if row_of:
        r["row_of"] = np.zeros(max(n, 1), np.uint32)
    i = N.KeyedEvents()
    i.n, i.device, i.key = n, device, _p(key, C.c_int32)
    if packed:
        i.ev_word, i.process = _p(ev[0], C.c_uint32), _p(ev[1], C.c_int32)
    else:
        i.type, i.process, i.f, i.a, i.b = _p(ev.type, C.c_uint8), _p(ev.process, C.c_int32), _p(ev.f, C.c_uint8), _p(ev.a, C.c_int32), _p(ev.b, C.c_int32)
    s = N.SplitOut()
    s.keys_cap, s.keys, s.ev_off = kc, _p(r["keys"], C.c_int32), _p(r["ev_off"], C.c_uint64)
    if row_of:
        s.row_of = _p(r["row_of"], C.c_uint32)
    o = None
    if pair:
        nh = max(kc, 1)
        r.update(status=np.zeros(nh, np.int32), bad_row=np.zeros(nh, np.uint32), op_off=np.zeros(kc + 1, np.uint64), n_events=np.zeros(nh, np.uint32),
                 n_process=np.zeros(nh, np.uint32), inv_pos=np.zeros(m, np.uint32), ret_pos=np.zeros(m, np.uint32))
        if word:
            r["word"] = np.zeros(m, np.uint32)
        if columns:
            r.update(f=np.zeros(m, np.uint8), a=np.zeros(m, np.int32), b=np.zeros(m, np.int32), process=np.zeros(m, np.int32))
        o = N.PairOut()
        o.ops_cap = cap
        for name, ct in (("op_off", C.c_uint64), ("n_events", C.c_uint32), ("n_process", C.c_uint32), ("f", C.c_uint8), ("a", C.c_int32),
                         ("b", C.c_int32), ("process", C.c_int32), ("inv_pos", C.c_uint32), ("ret_pos", C.c_uint32), ("word", C.c_uint32),
                         ("status", C.c_int32), ("bad_row", C.c_uint32)):
            if name in r:
                setattr(o, name, _p(r[name], ct))
    st = (call or N.lib().tbc_pair_keyed_events)(C.byref(i), C.byref(s), C.byref(o) if pair else None)
    nk = int(s.n_keys) if st == N.OK_STATUS else 0
    r["n_keys"] = nk
    r["keys"], r["ev_off"] = r["keys"][:nk], r["ev_off"][:nk + 1]
    if row_of:
        r["row_of"] = r["row_of"][:n]
    if pair:
        r.update(n_bad=int(o.n_bad), n_ops=int(o.n_ops), ns_device=int(o.ns_device), bytes_in=int(o.bytes_in))
        for k in ("status", "bad_row", "n_events", "n_process"):
            r[k] = r[k][:nk]
        r["op_off"] = r["op_off"][:nk + 1]
    return st, r


def pair_keyed_events(ev: EventColumns, key, device=0):
    """tbc_pair_keyed_events: one keyed event history -> (keys int32[n_keys] by first appearance; a list of OpColumns, one per key,
    None where the key's history is refused; status int32[n_keys]; bad_row uint32[n_keys], a row WITHIN the key's rows, PAIR_NO_ROW
    where there is none; row_of uint32[n]: the original row of every split row, key after key -- split_events' row_of)."""
    st, r = pair_keyed_events_raw(ev, key, device=device)
    N.check_status(st)
    return r["keys"], keyed_ops(r), r["status"], r["bad_row"], r["row_of"]


def keyed_ops(r):
    """the OpColumns of every key out of what pair_keyed_events_raw returned (all six op columns asked for); None for a refused key"""
    ops = []
    for h in range(r["n_keys"]):
        if r["status"][h] != N.OK_STATUS:
            ops.append(None)
            continue
        lo, hi = int(r["op_off"][h]), int(r["op_off"][h + 1])
        ops.append(OpColumns(*[r[k][lo:hi].copy() for k in ("f", "a", "b", "process", "inv_pos", "ret_pos")],
                             n_events=int(r["n_events"][h]), n_process=int(r["n_process"][h])))
    return ops

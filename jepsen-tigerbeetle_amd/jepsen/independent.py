"""jepsen.independent -- tuple values and the per-key checker.

The reference wraps its set-full checkers this way
(workloads/set_full.clj:29-31,42-45 build [k v] tuples; :155 wraps the
checker).  Keys are independent objects, so each key's sub-history is
checked on its own (P-compositionality) -- and when the wrapped checker is the
GPU linearizability checker, ALL keys go to the device in one batch launch
(tbc_batch_*), one history per wavefront.
"""
from __future__ import annotations

from .. import _native as N
from .. import core
from ..knossos import _analysis
from . import checker as jc


class Tuple(tuple):
    """(independent/tuple k v)"""

    def __new__(cls, k, v):
        return super().__new__(cls, (k, v))

    key = property(lambda self: self[0])
    value = property(lambda self: self[1])


def tuple_(k, v):
    return Tuple(k, v)


def tuple_p(x):
    return isinstance(x, Tuple)


def history_keys(history):
    keys = []
    seen = set()
    for op in history:
        v = op.get("value")
        if tuple_p(v) and v.key not in seen:
            seen.add(v.key)
            keys.append(v.key)
    return keys


def subhistory(k, history):
    """Ops of key k with the tuple stripped; non-tuple ops (nemesis ...) are kept for every key."""
    out = []
    for op in history:
        v = op.get("value")
        if tuple_p(v):
            if v.key == k:
                out.append(dict(op, value=v.value))
        else:
            out.append(op)
    return out


def split(history):
    """(keys in order of first appearance, {k: subhistory(k, history)}) in ONE walk of the history: the same ops in the same order
    per key -- a tuple op as a copy with the tuple stripped, every non-tuple op (the same dict) in every key's sub-history, those
    before the key's first op included."""
    keys, subs, shared = [], {}, []
    for op in history:
        v = op.get("value")
        if tuple_p(v):
            sub = subs.get(v.key)
            if sub is None:
                sub = subs[v.key] = list(shared)
                keys.append(v.key)
            sub.append(dict(op, value=v.value))
        else:
            shared.append(op)
            for sub in subs.values():
                sub.append(op)
    return keys, subs


def _set_full_members(inner):
    """{name: checker} when `inner` is what the keyed set-full path answers (set-full, or a compose of set-full, read-all-invoked-adds
    and linearizable members), else None.  A bare SetFull is {None: it}."""
    if isinstance(inner, jc.SetFull):
        return {None: inner}
    if isinstance(inner, jc.Compose) and inner.checkers and any(isinstance(c, jc.SetFull) for c in inner.checkers.values()) and all(
            isinstance(c, (jc.SetFull, jc.ReadAllInvokedAdds, jc.Linearizable)) for c in inner.checkers.values()):
        return dict(inner.checkers)
    return None


class IndependentChecker(jc.Checker):
    def __init__(self, inner):
        self.inner = inner

    def check(self, test, history, opts=None):
        keys, subs = split(history)
        members = _set_full_members(self.inner)
        if isinstance(self.inner, jc.Linearizable) and keys:
            results = self._check_batched(keys, subs)
        elif members is not None and keys:
            results = self._check_set_full(keys, subs, members, opts)
        else:
            results = {k: self.inner.check(test, subs[k], opts) for k in keys}
        failures = [k for k in keys if results[k].get("valid?") is False]
        return {"valid?": jc.merge_valid(r.get("valid?") for r in results.values()),
                "results": results, "failures": failures}

    def _check_set_full(self, keys, subs, members, opts):
        """set-full (alone or composed, set_full.clj:155-158) over all keys: every key encoded once, every key's matrix scanned in one
        device pass and decided there (jepsen/set_full.py results_keys), each set-full member's result map from that, read-all-invoked-adds from
        the same encoding, linearizable members as one batch.  Per key what Compose.check / SetFull.check give on its sub-history."""
        from . import set_full as sf
        encs = {k: sf.Encoded(subs[k]) for k in keys}
        # (one scan and one deciding pass per :linearizable? value among the set-full members -- the flag is the device's to apply)
        devs = {flag: sf.results_keys(encs, flag, device=(opts or {}).get("device", 0))
                for flag in sorted({c.linearizable for c in members.values() if isinstance(c, jc.SetFull)})}
        lin = {name: IndependentChecker(c)._check_batched(keys, subs) for name, c in members.items() if isinstance(c, jc.Linearizable)}
        out = {}
        for k in keys:
            res = {}
            for name, c in members.items():
                if isinstance(c, jc.SetFull):
                    res[name] = sf.result_from_device(encs[k], devs[c.linearizable][k])
                elif isinstance(c, jc.ReadAllInvokedAdds):
                    res[name] = sf.read_all_invoked_adds(subs[k], encs[k])
                else:
                    res[name] = lin[name][k]
            if None in res:                                 # a bare set-full, not a compose
                out[k] = res[None]
                continue
            res["valid?"] = jc.merge_valid(r.get("valid?") for r in res.values() if isinstance(r, dict))
            out[k] = res
        return out

    def _check_batched(self, keys, subs):
        lin = self.inner
        shared = None
        if isinstance(lin.model, (_analysis.M.Register, _analysis.M.CASRegister)):
            # ONE model struct serves the whole batch: intern the values of all keys together, so that the encoded
            # initial value (and every other value) means the same thing in every key's columns
            shared = [v for k in keys for v in _analysis.register_values(subs[k])]
        encs = [_analysis.Encoded(lin.model, subs[k], shared_values=shared) for k in keys]
        kinds = {e.native_model[0].kind for e in encs}
        if (len(kinds) != 1 or N.MODEL_TABLE in kinds or len({e.native_model[0].n_keys for e in encs}) != 1
                or len({e.native_model[0].init for e in encs}) != 1 and N.MODEL_SET not in kinds and N.MODEL_BANK not in kinds):
            # table models have one table per key, and keys that do not agree on the encoded model: one by one
            return {k: lin.check(None, subs[k], None) for k in keys}
        want_witness = bool(lin.opts.get("witness", lin.algorithm == "wgl"))
        o = _analysis.make_opts_from(lin.algorithm, lin.opts, want_witness)
        with core.Batch([e.ops for e in encs], encs[0].native_model, o) as b:
            b.run(tolerate_bad_histories=True)
            res = b.results()
        out = {}
        for k, e, r in zip(keys, encs, res):
            if r["valid"] == N.UNKNOWN and r["cause"] == N.CAUSE_NONE:
                # rejected by the device-side validation (malformed rows): this key only, not the batch
                out[k] = {"valid?": "unknown", "cause": "malformed-history", "analyzer": "wgl", "configs": [], "final-paths": []}
                continue
            a = _analysis.result_map(e, r, lin.algorithm)
            a["final-paths"] = a["final-paths"][:10]
            a["configs"] = a["configs"][:10]
            out[k] = a
        return out


    def check_columns(self, ev, key, opts=None):
        """check() for a history that is already COLUMNS: `ev` (columns.EventColumns: the client ops of every key, the tuples stripped,
        register values as the small integers the device takes, N.NIL for nil) and key int32[len(ev)], the key of every row.  For a
        Linearizable inner over a register or cas-register whose initial value is such an integer (or None).  The history is split by key
        and paired per key on the device (columns.pair_keyed_events), the keys go to ONE core.Batch, and the result has the shape
        check() gives: {key: result} as _check_batched makes it, the ops rebuilt from the rows (their :index is the row of `ev`).
        Rows that belong to every key (nemesis ops) are the caller's to leave out.  The split and the pairing touch no op on the host; the batch is still created from the op columns that
        come back (core.Batch.stream_keyed_events is the route that keeps them on the device, for a batch that exists already)."""
        from .. import columns
        lin = self.inner
        if not isinstance(lin, jc.Linearizable) or not isinstance(lin.model, (_analysis.M.Register, _analysis.M.CASRegister)):
            raise ValueError("check_columns: a Linearizable checker over a register or cas-register")
        device = (opts or {}).get("device", lin.opts.get("device", 0))
        st, raw = columns.pair_keyed_events_raw(ev, key, device=device)      # (pair_keyed_events, with the device's ev_off kept)
        N.check_status(st)
        keys, ops, row_of, offs, results = [int(k) for k in raw["keys"]], columns.keyed_ops(raw), raw["row_of"], raw["ev_off"].astype("int64"), {}
        good = [k for k in range(len(keys)) if ops[k] is not None]
        res = []
        if good:
            kind = N.MODEL_CAS_REGISTER if isinstance(lin.model, _analysis.M.CASRegister) else N.MODEL_REGISTER
            init = N.NIL if lin.model.value is None else int(lin.model.value)
            want_witness = bool(lin.opts.get("witness", lin.algorithm == "wgl"))
            with core.Batch([ops[k] for k in good], core.make_model(kind, init), _analysis.make_opts_from(lin.algorithm, lin.opts, want_witness)) as b:
                b.run(tolerate_bad_histories=True)
                res = b.results()
        by_key = dict(zip(good, res))
        for k, name in enumerate(keys):
            r = by_key.get(k)
            if r is None or (r["valid"] == N.UNKNOWN and r["cause"] == N.CAUSE_NONE):
                results[name] = {"valid?": "unknown", "cause": "malformed-history", "analyzer": "wgl", "configs": [], "final-paths": []}
                continue
            a = _analysis.result_map(_ColumnsEncoded(lin.model, ops[k], _KeyRows(ev, row_of[offs[k]:offs[k + 1]])), r, lin.algorithm)
            a["final-paths"] = a["final-paths"][:10]
            a["configs"] = a["configs"][:10]
            results[name] = a
        failures = [k for k in keys if results[k].get("valid?") is False]
        return {"valid?": jc.merge_valid(r.get("valid?") for r in results.values()), "results": results, "failures": failures}


class _KeyRows:
    """row r of a key's sub-history as the op map it stands for, made when it is asked for"""
    _TYPE = {N.INVOKE: "invoke", N.OK: "ok", N.FAIL: "fail", N.INFO: "info"}
    _F = {N.F_READ: "read", N.F_WRITE: "write", N.F_CAS: "cas"}

    def __init__(self, ev, rows):
        self.ev, self.rows = ev, rows

    def __getitem__(self, r):
        at = int(self.rows[r])
        dec = lambda x: None if x == N.NIL else int(x)
        f = int(self.ev.f[at])
        a, b = dec(self.ev.a[at]), dec(self.ev.b[at])
        return {"index": at, "type": self._TYPE.get(int(self.ev.type[at])), "process": int(self.ev.process[at]), "f": self._F.get(f, f),
                "value": (None if a is None and b is None else (a, b)) if f == N.F_CAS else a}


class _ColumnsEncoded(_analysis.Encoded):
    """what _analysis.result_map reads of an Encoded, over columns: the values are their own encoding"""

    class _Identity:
        @staticmethod
        def dec(x):
            return None if x == N.NIL else int(x)

    def __init__(self, model, ops, rows):
        self.model, self.ops, self.rows, self.table_info, self.intern = model, ops, rows, None, self._Identity


def checker(inner):
    return IndependentChecker(inner)

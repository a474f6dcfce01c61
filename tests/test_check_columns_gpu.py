"""IndependentChecker.check_columns on the MI355X: one keyed history as columns -- split by key and paired on the device
(tbc_pair_keyed_events), the keys in one core.Batch -- against IndependentChecker.check on the same history as op maps with
independent tuples: the keys, every key's verdict, the op an invalid key fails at and the one before it.  16 keys of 200 ops, some
of them corrupted into invalid histories, one malformed."""
import numpy as np
import pytest

import keyed_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, synth
from jepsen_tigerbeetle_amd.jepsen import checker as jc, independent
from jepsen_tigerbeetle_amd.knossos import model as M

pytestmark = pytest.mark.gpu

TYPES = {N.INVOKE: "invoke", N.OK: "ok", N.FAIL: "fail", N.INFO: "info"}
FS = {N.F_READ: "read", N.F_WRITE: "write", N.F_CAS: "cas"}


def keyed_history(malformed=False):
    evs = [synth.register_events(n_ops=200, n_procs=5, seed=900 + k, busy=0.3, info=0.02 if k % 3 == 0 else 0.0, corrupt=0.4 if k % 4 == 1 else 0.0) for k in range(16)]
    if malformed:
        evs[6].type[11] = N.OK if evs[6].type[11] == N.INVOKE else N.INVOKE
    return S.interleave(evs, [1000 - 37 * k for k in range(16)])


def op_maps(ev, key):
    dec = lambda x: None if x == N.NIL else int(x)
    out = []
    for r in range(len(ev)):
        f, a, b = int(ev.f[r]), dec(ev.a[r]), dec(ev.b[r])
        v = (None if a is None and b is None else (a, b)) if f == N.F_CAS else a
        out.append({"type": TYPES[int(ev.type[r])], "process": int(ev.process[r]), "f": FS[f], "value": independent.tuple_(int(key[r]), v)})
    return out


def same_op(a, b):
    if a is None or b is None:
        return a is None and b is None
    va, vb = a.get("value"), b.get("value")
    return (a["type"], a["process"], a["f"]) == (b["type"], b["process"], b["f"]) and (tuple(va) if isinstance(va, (list, tuple)) else va) == (tuple(vb) if isinstance(vb, (list, tuple)) else vb)


@pytest.mark.parametrize("algorithm", ["wgl", "linear"])
def test_check_columns_equals_check(native, algorithm):
    ev, key = keyed_history()
    chk = independent.checker(jc.linearizable({"model": M.cas_register(None), "algorithm": algorithm}))
    got, want = chk.check_columns(ev, key), chk.check(None, op_maps(ev, key))
    assert list(got["results"]) == list(want["results"]) and len(got["results"]) == 16
    assert got["valid?"] == want["valid?"] and got["failures"] == want["failures"]
    verdicts = [r["valid?"] for r in want["results"].values()]
    assert True in verdicts and False in verdicts
    for k, w in want["results"].items():
        g = got["results"][k]
        assert g["valid?"] == w["valid?"] and g["analyzer"] == w["analyzer"], k
        if w["valid?"] is False:
            assert same_op(g["op"], w["op"]) and same_op(g["previous-ok"], w["previous-ok"]), (k, g["op"], w["op"])
            assert key[g["op"]["index"]] == k                       # (:index is the row of the one history)
            assert len(g["configs"]) == len(w["configs"]) and len(g["final-paths"]) == len(w["final-paths"])


def test_a_malformed_key_costs_itself(native):
    ev, key = keyed_history(malformed=True)
    chk = independent.checker(jc.linearizable({"model": M.cas_register(None), "algorithm": "wgl"}))
    got = chk.check_columns(ev, key)
    bad = 1000 - 37 * 6
    assert got["results"][bad] == {"valid?": "unknown", "cause": "malformed-history", "analyzer": "wgl", "configs": [], "final-paths": []}
    clean = chk.check_columns(*keyed_history())
    for k, r in clean["results"].items():
        if k != bad:
            assert got["results"][k]["valid?"] == r["valid?"], k
    with pytest.raises(ValueError):
        independent.checker(jc.SetFull()).check_columns(ev, key)

"""set-full over many keys in one device pass (tbc_setfull_keys_*, csrc/set_full.hip) and the reference's composed checker
(workloads/set_full.clj:155-158: independent/checker over compose {:set-full (set-full {:linearizable? true}),
:read-all-invoked-adds (read-all-invoked-adds)}).  CPU: the one-walk key split, read-all-invoked-adds against a plain set
restatement, the new structs' layout, host validation of the keyed input, no CPU fallback.  GPU: the keyed scan equals the
single-key scan and the restatement key by key, bit for bit; the budget split; the composed checker key by key and on the
EDN goldens; reruns and two objects from two threads."""
import ctypes as C
import json
import os
import random
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from helpers import GOLDEN, set_history
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.columns import _p
from jepsen_tigerbeetle_amd.jepsen import checker as jc, edn, independent, set_full as sf
from oracle import set_full as osf

NONE = N.NO_OP
T = independent.tuple_


# ---------------------------------------------------------------------------------------------------- histories
def _keyed(hists, nemesis_every=0, seed=0):
    """{k: history} interleaved into one independent history (processes kept apart per key), nemesis ops sprinkled in."""
    rng = random.Random(seed)
    queues = {k: [dict(o, value=T(k, o["value"]), process=o["process"] * 1000 + i) for o in h] for i, (k, h) in enumerate(hists.items())}
    out = []
    while any(queues.values()):
        k = rng.choice([k for k, q in queues.items() if q])
        out.append(queues[k].pop(0))
        if nemesis_every and rng.random() < 1.0 / nemesis_every:
            out.append({"type": "info", "f": "start-partition", "value": None, "process": "nemesis"})
    return [dict(o, index=i) for i, o in enumerate(out)]


def _with_final_reads(hist, n_procs, seed, drop=0):
    """`hist` plus one :final? read per process at the end (as the reference's final generator issues them), each returning the set
    of every acknowledged add -- minus `drop` random ones, and crashed adds as they happened to land."""
    rng = random.Random(seed)
    acked = sorted(o["value"] for o in hist if o["f"] == "add" and o["type"] == "ok")
    crashed = [o["value"] for o in hist if o["f"] == "add" and o["type"] == "info"]
    out = list(hist)
    procs = sorted({o["process"] for o in hist if isinstance(o["process"], int)}) or list(range(n_procs))
    for p in procs[:3]:
        seen = [v for v in acked if rng.random() >= (drop / max(1, len(acked)))] + [v for v in crashed if rng.random() < 0.5]
        out.append({"type": "invoke", "f": "read", "value": None, "process": p + 10_000, "final?": True})
        out.append({"type": "ok", "f": "read", "value": sorted(seen), "process": p + 10_000, "final?": True})
    return [dict(o, index=i) for i, o in enumerate(out)]


def _raia_restated(history):
    """read-all-invoked-adds restated as plain sets (workloads/set_full.clj:51-75)."""
    adds = {o["value"] for o in history if o.get("f") == "add" and o.get("type") == "invoke"}
    bad = []
    for i, o in enumerate(history):
        if o.get("f") == "read" and o.get("type") == "ok" and o.get("final?"):
            miss = adds - set(o.get("value") or [])
            if miss:
                bad.append([i, sorted(miss)])
    return {"valid?": False, "suspect-final-reads": bad} if bad else {"valid?": True}


def _h(rows):
    return [dict({"type": t, "f": f, "value": v, "process": p, "index": i}, **(x[0] if x else {})) for i, (t, f, v, p, *x) in enumerate(rows)]


# ---------------------------------------------------------------------------------------------------- CPU tier
def test_split_equals_subhistory_for_every_key():
    sizes = {"big": 900, 7: 40, ("t", 1): 6, 3.5: 200}
    hists = {k: set_history(n, 4, s, busy=0.3, info=0.05) for s, (k, n) in enumerate(sizes.items())}
    only_adds = [o for o in set_history(60, 3, 9) if o["f"] == "add"]
    only_reads = [o for o in set_history(60, 3, 10) if o["f"] == "read"]
    words = [dict(o, value=("w%d" % o["value"]) if o["f"] == "add" else (["w%d" % x for x in o["value"]] if o["value"] else o["value"]))
             for o in set_history(80, 3, 11)]
    hists.update({"adds": only_adds, "reads": only_reads, "words": words})
    for seed in range(3):
        hist = _keyed(hists, nemesis_every=7, seed=seed)
        hist.insert(0, {"type": "info", "f": "start", "value": None, "process": "nemesis"})       # before any key's first op
        keys, subs = independent.split(hist)
        assert keys == independent.history_keys(hist)
        assert set(subs) == set(keys)
        for k in keys:
            assert subs[k] == independent.subhistory(k, hist), k
            assert [id(o) for o in subs[k] if not independent.tuple_p(o.get("value")) and o.get("process") == "nemesis"] == \
                   [id(o) for o in hist if o.get("process") == "nemesis"]
    assert independent.split([]) == ([], {})


def test_read_all_invoked_adds_hand_cases():
    raia = jc.read_all_invoked_adds()
    fin = {"final?": True}
    # a final read missing an acknowledged add
    h = _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "add", 2, 0), ("ok", "add", 2, 0),
            ("invoke", "read", None, 1, fin), ("ok", "read", [1], 1, fin)])
    assert raia.check({}, h) == {"valid?": False, "suspect-final-reads": [[5, [2]]]}
    # a crashed add no final read saw is suspect, as in the reference; a non-final read missing everything is ignored
    h = _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "add", 2, 2), ("info", "add", 2, 2),
            ("invoke", "read", None, 1), ("ok", "read", [], 1), ("invoke", "read", None, 1, fin), ("ok", "read", [1, 99], 1, fin)])
    assert raia.check({}, h) == {"valid?": False, "suspect-final-reads": [[7, [2]]]}
    # every invoked add seen (values read but never added do not count)
    h = _h([("invoke", "add", 1, 0), ("info", "add", 1, 0), ("invoke", "read", None, 1, fin), ("ok", "read", [1, 5], 1, fin)])
    assert raia.check({}, h) == {"valid?": True}
    # no adds at all; a nil final value
    assert raia.check({}, _h([("invoke", "read", None, 1, fin), ("ok", "read", None, 1, fin)])) == {"valid?": True}
    h = _h([("invoke", "add", 3, 0), ("ok", "add", 3, 0), ("invoke", "read", None, 1, fin), ("ok", "read", None, 1, fin)])
    assert raia.check({}, h) == {"valid?": False, "suspect-final-reads": [[3, [3]]]}
    # an element added twice is one invoked value
    h = _h([("invoke", "add", 4, 0), ("ok", "add", 4, 0), ("invoke", "add", 4, 0), ("ok", "add", 4, 0),
            ("invoke", "read", None, 1, fin), ("ok", "read", [], 1, fin), ("invoke", "read", None, 2, fin), ("ok", "read", [4], 2, fin)])
    assert raia.check({}, h) == {"valid?": False, "suspect-final-reads": [[5, [4]]]}
    assert sf.read_all_invoked_adds(h, sf.Encoded(h)) == raia.check({}, h)


def test_read_all_invoked_adds_against_a_set_restatement():
    """Generated histories with :final? reads appended: the direct scan and the answer from the set-full encoding's compact rows
    both equal the restatement."""
    n_suspect = 0
    for seed in range(300):
        rng = random.Random(seed)
        base = set_history(rng.randrange(0, 120), rng.randrange(1, 5), seed, busy=0.4, info=rng.choice((0.0, 0.1, 0.3)))
        h = _with_final_reads(base, 3, seed, drop=rng.choice((0, 0, 1, 3)))
        if seed % 7 == 0 and len(h) > 4:          # an unmatched :ok final read (its invoke lost): the encoding drops it
            h = [dict(o, index=i) for i, o in enumerate(h[:-2] + h[-1:])]
        want = _raia_restated(h)
        n_suspect += want["valid?"] is False
        assert sf.read_all_invoked_adds(h) == want, seed
        assert sf.read_all_invoked_adds(h, sf.Encoded(h)) == want, seed
    assert 30 < n_suspect < 300


def test_keyed_struct_layouts_match_header(native):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "tbcheck.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tbc_setfull_keys_in),
  offsetof(tbc_setfull_keys_in, n_keys), offsetof(tbc_setfull_keys_in, device), offsetof(tbc_setfull_keys_in, n_elements),
  offsetof(tbc_setfull_keys_in, n_reads), offsetof(tbc_setfull_keys_in, add_invoke), offsetof(tbc_setfull_keys_in, add_ok),
  offsetof(tbc_setfull_keys_in, read_invoke), offsetof(tbc_setfull_keys_in, read_ok), offsetof(tbc_setfull_keys_in, top),
  offsetof(tbc_setfull_keys_in, exc_off), offsetof(tbc_setfull_keys_in, exc),
  sizeof(tbc_setfull_keys_out), offsetof(tbc_setfull_keys_out, known), offsetof(tbc_setfull_keys_out, last_present),
  offsetof(tbc_setfull_keys_out, last_absent), offsetof(tbc_setfull_keys_out, ns_scan), offsetof(tbc_setfull_keys_out, bytes_scanned),
  offsetof(tbc_setfull_keys_out, bytes_matrix)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "k.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "k")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    I, O = native.SetFullKeysIn, native.SetFullKeysOut
    mine = [C.sizeof(I)] + [getattr(I, f).offset for f, _ in I._fields_] + [C.sizeof(O)] + [getattr(O, f).offset for f, _ in O._fields_]
    assert mine == got
    for name in ("tbc_setfull_keys_create", "tbc_setfull_keys_run", "tbc_setfull_keys_destroy"):
        assert name in native.SYMBOLS and hasattr(native.lib(), name)


class _Arr:
    """A key's inputs in the encoder's compact form, built directly."""


def _synthetic_key(E, R, seed, shuffle_exc=False):
    """E elements, R reads of a grow-only set: each read holds a prefix of what had been invoked when it completed (top), a few holes
    below it and a few elements above it (both as exceptions), in ascending order or shuffled."""
    rng = np.random.default_rng(seed)
    a = _Arr()
    a.E, a.R = E, R
    a.wpr = max(1, (E + 31) // 32)
    t = 1 + np.cumsum(rng.integers(1, 4, E + R))            # one timeline for adds and reads
    kind = np.zeros(E + R, bool)
    kind[rng.choice(E + R, R, replace=False)] = True         # True = a read starts here
    a.add_invoke = (t[~kind] * 4).astype(np.uint32)
    a.add_ok = np.where(rng.random(E) < 0.9, a.add_invoke + 1 + 4 * rng.integers(0, 3, E), NONE).astype(np.uint32)
    a.read_invoke = (t[kind] * 4 + 2).astype(np.uint32)
    a.read_ok = (a.read_invoke + 1 + 4 * rng.integers(0, 6, R)).astype(np.uint32)
    invoked = np.searchsorted(a.add_invoke, a.read_ok)       # elements whose add was invoked before the read completed
    a.top = np.minimum(E, invoked + rng.integers(0, 2, R)).astype(np.uint32) if R else np.zeros(1, np.uint32)
    parts, off = [], [0]
    for r in range(R):
        tp = int(a.top[r])
        holes = rng.choice(tp, min(tp, int(rng.integers(0, 4))), replace=False) if tp else np.zeros(0, np.int64)
        above = rng.choice(E - tp, min(E - tp, int(rng.integers(0, 2))), replace=False) + tp if E > tp else np.zeros(0, np.int64)
        ex = np.concatenate([holes, above]).astype(np.uint32)
        ex = rng.permutation(ex) if shuffle_exc else np.sort(ex)
        parts.append(ex)
        off.append(off[-1] + len(ex))
    a.exc_off = np.array(off, np.uint64)
    a.exc = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return a


def _dense_states(a, block_cells=4_000_000):
    """known / last-present / last-absent by a numpy reduction over the dense matrix (only reads completing after the add count), a
    block of rows x columns of at most `block_cells` cells at a time (the reductions are a max and two mins: blocks combine exactly)."""
    E, R = a.E, a.R
    lp, la, kn = np.full(E, -1, np.int64), np.full(E, -1, np.int64), np.full(E, 2 ** 40, np.int64)
    cols = max(1, min(E, 8192))
    rows = max(1, min(R, block_cells // cols))
    exc_row = np.repeat(np.arange(R, dtype=np.int64), np.diff(a.exc_off.astype(np.int64)))
    exc = a.exc.astype(np.int64)
    for r0 in range(0, R, rows):
        r1 = min(R, r0 + rows)
        x0, x1 = int(a.exc_off[r0]), int(a.exc_off[r1])
        inv, ok = a.read_invoke[r0:r1].astype(np.int64)[:, None], a.read_ok[r0:r1].astype(np.int64)[:, None]
        for c0 in range(0, E, cols):
            c1 = min(E, c0 + cols)
            pres = np.arange(c0, c1, dtype=np.int64)[None, :] < a.top[r0:r1].astype(np.int64)[:, None]
            m = (exc[x0:x1] >= c0) & (exc[x0:x1] < c1)
            pres[exc_row[x0:x1][m] - r0, exc[x0:x1][m] - c0] ^= True          # (each element at most once per read: no pair twice)
            counts = a.add_invoke[None, c0:c1].astype(np.int64) < ok
            lp[c0:c1] = np.maximum(lp[c0:c1], np.where(pres & counts, inv, -1).max(axis=0, initial=-1))
            la[c0:c1] = np.maximum(la[c0:c1], np.where(~pres & counts, inv, -1).max(axis=0, initial=-1))
            kn[c0:c1] = np.minimum(kn[c0:c1], np.where(pres & counts, ok, 2 ** 40).min(axis=0, initial=2 ** 40))
    kn = np.minimum(kn, a.add_ok.astype(np.int64))
    u = lambda x, big: np.where((x < 0) | (x >= big), NONE, x).astype(np.uint32)
    return {"known": u(np.where(kn == NONE, 2 ** 40, kn), 2 ** 40), "last_present": u(lp, 2 ** 40), "last_absent": u(la, 2 ** 40)}


def _keys_in(arrs):
    """A tbc_setfull_keys_in over `arrs` (and the arrays it points into)."""
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt) for x in xs] + [np.zeros(1, dt)]), dt)
    keep = dict(E=np.array([a.E for a in arrs], np.uint32), R=np.array([a.R for a in arrs], np.uint32),
                ai=cat([a.add_invoke for a in arrs], np.uint32), ao=cat([a.add_ok for a in arrs], np.uint32),
                ri=cat([a.read_invoke for a in arrs], np.uint32), ro=cat([a.read_ok for a in arrs], np.uint32),
                top=cat([a.top[:a.R] for a in arrs], np.uint32), exc=cat([a.exc for a in arrs], np.uint32))
    offs, base = [np.zeros(1, np.uint64)], 0
    for a in arrs:
        offs.append(np.asarray(a.exc_off[1:], np.uint64) + np.uint64(base))
        base += int(a.exc_off[-1])
    keep["off"] = np.ascontiguousarray(np.concatenate(offs), np.uint64)
    s = N.SetFullKeysIn()
    s.n_keys, s.device = len(arrs), 0
    s.n_elements, s.n_reads = _p(keep["E"], C.c_uint32), _p(keep["R"], C.c_uint32)
    s.add_invoke, s.add_ok = _p(keep["ai"], C.c_uint32), _p(keep["ao"], C.c_uint32)
    s.read_invoke, s.read_ok = _p(keep["ri"], C.c_uint32), _p(keep["ro"], C.c_uint32)
    s.top, s.exc_off, s.exc = _p(keep["top"], C.c_uint32), _p(keep["off"], C.c_uint64), _p(keep["exc"], C.c_uint32)
    return s, keep


def _create_status(arrs):
    s, keep = _keys_in(arrs)
    h = C.c_void_p()
    st = N.lib().tbc_setfull_keys_create(C.byref(s), C.byref(h))
    if st == 0:
        N.lib().tbc_setfull_keys_destroy(h)
    return st, N.lib().tbc_last_error().decode()


def test_bad_keyed_input_is_refused_on_the_host_naming_the_key(native):
    """Every rule is checked before any device work (so this holds with or without a GPU), and the message names the key."""
    good = [_synthetic_key(40, 30, s) for s in range(4)]
    dup = [_synthetic_key(40, 30, s) for s in range(4)]
    r = next(r for r in range(dup[2].R) if dup[2].exc_off[r + 1] - dup[2].exc_off[r] >= 1 and dup[2].top[r] >= 2)
    lo = int(dup[2].exc_off[r])
    x = int(dup[2].exc[lo])
    dup[2].exc = np.insert(dup[2].exc, lo, x)
    dup[2].exc_off = dup[2].exc_off.copy(); dup[2].exc_off[r + 1:] += 1
    st, msg = _create_status(dup)
    assert st == N.ERR_INVALID_ARG and "key 2" in msg and "read %d" % r in msg and "twice" in msg, msg
    high = [_synthetic_key(40, 30, s) for s in range(4)]
    high[1].top = high[1].top.copy(); high[1].top[5] = 41
    st, msg = _create_status(high)
    assert st == N.ERR_INVALID_ARG and "key 1 read 5" in msg and "top" in msg, msg
    uns = [_synthetic_key(40, 30, s) for s in range(4)]
    uns[3].add_invoke = uns[3].add_invoke.copy(); uns[3].add_invoke[[7, 8]] = uns[3].add_invoke[[8, 7]]
    st, msg = _create_status(uns)
    assert st == N.ERR_INVALID_ARG and "key 3" in msg and "add_invoke" in msg, msg
    out = [_synthetic_key(40, 30, s) for s in range(2)]
    out[0].exc = out[0].exc.copy()
    out[0].exc[0] = 40
    st, msg = _create_status(out)
    assert st == N.ERR_INVALID_ARG and "key 0" in msg, msg
    s, keep = _keys_in(good)
    s.n_keys = 0
    h = C.c_void_p()
    assert N.lib().tbc_setfull_keys_create(C.byref(s), C.byref(h)) == N.ERR_INVALID_ARG
    assert "n_keys" in N.lib().tbc_last_error().decode()
    assert sf.check_keys({}) == {}


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_keyed_paths_have_no_cpu_fallback(native):
    hists = {k: set_history(100, 3, k) for k in range(3)}
    with pytest.raises(N.NoDeviceError):
        sf.check_keys(hists, True)
    c = independent.checker(jc.compose({"set-full": jc.set_full({"linearizable?": True}), "read-all-invoked-adds": jc.read_all_invoked_adds()}))
    with pytest.raises(N.NoDeviceError):
        c.check({}, _keyed(hists), {})
    with pytest.raises(N.NoDeviceError):
        independent.checker(jc.set_full()).check({}, _keyed(hists), {})


# ---------------------------------------------------------------------------------------------------- GPU tier
def _single(a):
    with sf.Scan(a, rows=True) as s:
        st = s.run()
    return st


def test_blocked_dense_states_equal_the_unblocked_ones():
    """_dense_states is the keyed scan's independent partner on every key, the large ones block by block: blocks of any size give what
    one block over the whole matrix gives, and that is the oracle's answer on a history."""
    for E, R, seed, shuffle in ((0, 5, 1, False), (7, 0, 2, False), (1, 1, 3, False), (33, 129, 4, True), (129, 2049, 5, False), (5000, 300, 6, True)):
        a = _synthetic_key(E, R, seed, shuffle_exc=shuffle)
        whole = _dense_states(a, block_cells=1 << 62)
        for cells in (1, 1000, 100_000):
            part = _dense_states(a, block_cells=cells)
            for f in ("known", "last_present", "last_absent"):
                assert np.array_equal(part[f], whole[f]), (E, R, cells, f)
    h = set_history(1500, 5, 31, busy=0.3, info=0.02)
    d, want = _dense_states(sf.Encoded(h), block_cells=5000), osf.element_states(h)
    for f in ("known", "last_present", "last_absent"):
        assert [int(x) for x in d[f]] == [w[f] for w in want], f


def _assert_keyed_equals_single(arrs, dense_limit=None):
    """keyed == Scan(rows=True) key by key (many keys placed == one key placed: both share the host code) and, for every key of at most
    `dense_limit` cells (None: every key), == the numpy reduction, which shares nothing with either."""
    with sf.KeyedScan(arrs) as ks:
        per, tot = ks.run()
    assert len(per) == len(arrs)
    for i, (a, got) in enumerate(zip(arrs, per)):
        want = _single(a)
        for f in ("known", "last_present", "last_absent"):
            assert np.array_equal(got[f], want[f]), (i, a.E, a.R, f)
        if dense_limit is None or a.E * a.R <= dense_limit:
            d = _dense_states(a)
            for f in ("known", "last_present", "last_absent"):
                assert np.array_equal(got[f], d[f]), (i, a.E, a.R, f, "numpy")
    return per, tot


@pytest.mark.gpu
def test_keyed_equals_single_key_on_histories(native):
    """One key, then config 3's shape (5 keys, ~50k ops): keyed == single-key Scan(rows=True) == oracle element_states."""
    for hists in ({0: set_history(3000, 8, 1, busy=0.3, info=0.02)},
                  {k: set_history(10_000, 10, 40 + k, busy=0.3, info=0.02, corrupt="lost" if k == 2 else None) for k in range(5)}):
        encs = [sf.Encoded(h) for h in hists.values()]
        per, _ = _assert_keyed_equals_single(encs, dense_limit=0)
        for h, got in zip(hists.values(), per):
            want = osf.element_states(h)
            assert [int(x) for x in got["known"]] == [w["known"] for w in want]
            assert [int(x) for x in got["last_present"]] == [w["last_present"] for w in want]
            assert [int(x) for x in got["last_absent"]] == [w["last_absent"] for w in want]


@pytest.mark.gpu
def test_keyed_equals_single_key_on_every_edge_shape(native):
    """~300 keys, E in {0, 1, 31, 32, 33, 127, 128, 129, 5000, 70000} x R in {0, 1, 2049, 5000}, exceptions ascending or shuffled,
    next to one key whose reads span more than 256 chunks of 2,048."""
    Es, Rs = (0, 1, 31, 32, 33, 127, 128, 129, 5000, 70000), (0, 1, 2049, 5000)
    arrs = []
    for rep in range(7):
        for E in Es:
            for R in Rs:
                if E == 70000 and R and rep > 1:
                    R = 1 + rep                                   # (keep the arena modest: two reps of the big ones)
                arrs.append(_synthetic_key(E, R, 1000 * rep + 7 * E + R, shuffle_exc=(rep % 2 == 1)))
    random.Random(3).shuffle(arrs)
    long = _synthetic_key(64, 2048 * 256 + 3000, 77)
    arrs.insert(len(arrs) // 2, long)
    assert len(arrs) >= 280
    _assert_keyed_equals_single(arrs)


@pytest.mark.gpu
def test_budget_split_gives_the_same_results(native, monkeypatch):
    hists = {k: set_history(2000 + 500 * k, 6, 70 + k, busy=0.3) for k in range(7)}
    whole = sf.check_keys(hists, True)
    calls = []
    real = sf.KeyedScan

    class Counting(real):
        def __init__(self, encs, device=0):
            encs = list(encs)
            calls.append(len(encs))
            super().__init__(encs, device)

    monkeypatch.setattr(sf, "KeyedScan", Counting)
    monkeypatch.setattr(sf, "KEYS_BUDGET_BYTES", max(sf._matrix_bytes(sf.Encoded(h)) for h in hists.values()))
    split = sf.check_keys(hists, True)
    assert len(calls) >= 3 and sum(calls) == len(hists)
    assert split == whole
    for k, h in hists.items():
        assert whole[k] == sf.check(h, True), k


def _composed():
    return jc.compose({"set-full": jc.set_full({"linearizable?": True}), "read-all-invoked-adds": jc.read_all_invoked_adds()})


@pytest.mark.gpu
def test_reference_composition_key_by_key(native):
    hists = {}
    for k in range(6):
        h = set_history(1200 + 300 * k, 5, 90 + k, busy=0.3, info=0.05, corrupt="lost" if k == 4 else None)
        hists[k] = _with_final_reads(h, 5, k, drop=1 if k in (1, 4) else 0)
    hists["empty-reads"] = [o for o in set_history(200, 3, 99) if o["f"] == "add"]
    hist = _keyed(hists, nemesis_every=11, seed=1)
    got = independent.checker(_composed()).check({}, hist, {})
    keys, subs = independent.split(hist)
    assert list(got["results"]) == keys
    for k in keys:
        want = _composed().check({}, subs[k], {})
        assert got["results"][k] == want, k
        o = osf.check(subs[k], True)
        for f in ("valid?", "attempt-count", "stable-count", "lost", "never-read", "stale"):
            assert got["results"][k]["set-full"][f] == o[f], (k, f)
        assert got["results"][k]["read-all-invoked-adds"] == _raia_restated(subs[k]), k
    assert got["valid?"] is False and got["results"][1]["read-all-invoked-adds"]["valid?"] is False
    # a bare set-full under independent: one keyed pass too, the same maps
    bare = independent.checker(jc.set_full({"linearizable?": False})).check({}, hist, {})
    assert bare["results"] == {k: sf.check(subs[k], False) for k in keys}


@pytest.mark.gpu
def test_reference_composition_on_the_edn_goldens(native):
    d = os.path.join(GOLDEN, "edn_checkers")
    cases = [c for c in json.load(open(os.path.join(d, "expected.json")))["cases"] if c["checker"] == "set-full"]
    files = sorted({c["file"] for c in cases})
    hists = {f: edn.read_history(os.path.join(d, f)) for f in files}
    hist = [dict(o, value=T(f, o["value"])) for f in files for o in hists[f]]
    hist = [dict(o, index=i) for i, o in enumerate(hist)]
    keys = ("valid?", "attempt-count", "stable-count", "lost-count", "lost", "never-read-count", "never-read", "stale-count", "stale", "duplicated-count")
    for lin in (True, False):
        c = independent.checker(jc.compose({"set-full": jc.set_full({"linearizable?": lin}), "read-all-invoked-adds": jc.read_all_invoked_adds()}))
        got = c.check({}, hist, {})
        seen = 0
        for case in cases:
            if case["opts"]["linearizable?"] is not lin:
                continue
            r = got["results"][case["file"]]["set-full"]
            for k in keys:
                assert r[k] == case["expect"][k], (case["file"], lin, k)
            assert {str(k): v for k, v in r["duplicated"].items()} == case["expect"]["duplicated"]
            seen += 1
        assert seen >= 6


@pytest.mark.gpu
def test_reruns_and_two_objects_from_two_threads(native):
    a = [sf.Encoded(set_history(3000, 6, 200 + k, busy=0.3)) for k in range(8)]
    b = [_synthetic_key(E, R, 300 + E) for E, R in ((5000, 2049), (33, 5000), (129, 1), (0, 7), (70000, 300))]
    with sf.KeyedScan(a) as ka, sf.KeyedScan(b) as kb:
        first = [ka.run()[0], kb.run()[0]]
        again = [ka.run()[0], kb.run()[0]]
        same = lambda x, y: all(np.array_equal(p[f], q[f]) for p, q in zip(x, y) for f in ("known", "last_present", "last_absent"))
        assert same(first[0], again[0]) and same(first[1], again[1])
        res = [[], []]
        th = [threading.Thread(target=lambda i=i, o=o: [res[i].append(o.run()[0]) for _ in range(4)]) for i, o in enumerate((ka, kb))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert len(res[0]) == len(res[1]) == 4
        assert all(same(r, first[0]) for r in res[0]) and all(same(r, first[1]) for r in res[1])

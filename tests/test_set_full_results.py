"""set-full's check result decided on the device (tbc_setfull_results / tbc_setfull_keys_results, csrc/set_full_results.h): outcome and
latencies per element, counts, :valid?, latency quantiles and worst stale elements per key.

CPU: the new structs' layout against gcc and the new symbols; the host builder of the result map (`result_from_device`) fed by a numpy
model of the device over the ORACLE's three indices, against oracle.set_full.check; no CPU fallback.
GPU: every value the library returns equals that numpy model over the oracle's / the numpy reduction's three indices, exactly -- edge
shapes, objects of 1 / 3 / 40 / 48 keys with empty keys, a key split across many workgroups, the three entry points, latency families
(zero, equal, clamped, above 32 bits, no :time), quantile ranks, worst-stale ties, every verdict; end to end through check, check_keys
and independent/checker; input rules; reruns, threads, run() after results()."""
import ctypes as C
import json
import os
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
from test_set_full import _lossy_set_history
from test_set_full_keys import _dense_states, _keyed, _synthetic_key

NONE = N.NO_OP
MS = 1_000_000


# ---------------------------------------------------------------------------------------------------- the numpy model of the device
def np_decide(known, lp, la, times, unit, linearizable):
    """What tbc_setfull_results must return for one key, from the three indices: numpy over whole columns for the per-element
    arrays, oracle.set_full._quantiles and a stable Python sort for the summary.  times None: the op index, unit 1."""
    known, lp, la = (np.asarray(x, np.uint32) for x in (known, lp, la))
    E = len(known)
    kn, hp, ha = known != NONE, lp != NONE, la != NONE
    k, lpi, lai = known.astype(np.int64), np.where(hp, lp.astype(np.int64), -1), np.where(ha, la.astype(np.int64), -1)
    stable = hp & (lai < lpi)
    lost = kn & ha & (lpi < lai) & (k < lai)
    if times is None:
        top = max([int(x.max()) for x, m in ((k[kn], kn), (lpi[hp], hp), (lai[ha], ha)) if m.any()] + [0])
        times, unit = np.arange(top + 1, dtype=np.int64), 1
    t = np.asarray(times, np.int64)
    at = lambda idx, has: t[np.where(has, idx, 0)] if len(t) else np.zeros(E, np.int64)
    tk = np.where(kn, at(k, kn), 0)
    t_la, t_lp = np.where(ha, at(lai, ha) + 1, 0), np.where(hp, at(lpi, hp) + 1, 0)
    slat = np.where(stable, np.maximum(0, t_la - tk) // unit, -1).astype(np.int64)
    llat = np.where(lost, np.maximum(0, t_lp - tk) // unit, -1).astype(np.int64)
    outcome = np.where(stable, N.SETFULL_STABLE, np.where(lost, N.SETFULL_LOST, N.SETFULL_NEVER_READ)).astype(np.uint8)
    stale = stable & (slat > 0)
    worst = sorted(np.nonzero(stale)[0].tolist(), key=lambda i: -int(slat[i]))[:8]
    q = lambda xs: [osf._quantiles(xs)[p] for p in (0, 0.5, 0.95, 0.99, 1)] if xs else None
    valid = False if lost.any() else ("unknown" if not stable.any() else (False if (linearizable and stale.any()) else True))
    summary = {"attempt_count": E, "stable_count": int(stable.sum()), "lost_count": int(lost.sum()),
               "never_read_count": int((~(stable | lost)).sum()), "stale_count": int(stale.sum()), "valid": valid,
               "stable_q": q([int(x) for x in slat[stable]]), "lost_q": q([int(x) for x in llat[lost]]),
               "worst": [{"element": i, "latency": int(slat[i]), "known": int(known[i]) if kn[i] else None,
                          "last_absent": int(la[i]) if ha[i] else None} for i in worst]}
    return {"outcome": outcome, "stable_latency": slat, "lost_latency": llat, "summary": summary}


def _assert_same(got, want, what):
    for f in ("outcome", "stable_latency", "lost_latency"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    assert got["summary"] == want["summary"], (what, got["summary"], want["summary"])


def _states_of(h):
    st = osf.element_states(h)
    return tuple(np.array([e[f] for e in st], np.uint32) for f in ("known", "last_present", "last_absent"))


def _timed(h, seed, step_ns=3 * MS):
    """The history with a :time on every op (ns, ascending by up to `step_ns` an op)."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.integers(1, step_ns, len(h)))
    return [dict(o, time=int(x)) for o, x in zip(h, t)]


def _edn_setfull_histories():
    d = os.path.join(GOLDEN, "edn_checkers")
    cases = [c for c in json.load(open(os.path.join(d, "expected.json")))["cases"] if c["checker"] == "set-full"]
    return {f: edn.read_history(os.path.join(d, f)) for f in sorted({c["file"] for c in cases})}


# ---------------------------------------------------------------------------------------------------- CPU tier
def test_results_struct_layouts_match_header_and_symbols_are_bound(native):
    structs = {"tbc_setfull_times": (native.SetFullTimes, ("op_time", "time_off", "unit", "flags", "reserved0")),
               "tbc_setfull_key_summary": (native.SetFullKeySummary, ("attempt_count", "stable_count", "lost_count", "never_read_count", "stale_count",
                                                                      "valid", "stable_q_present", "lost_q_present", "n_worst", "stable_q", "lost_q",
                                                                      "worst_element", "worst_known", "worst_last_absent", "worst_latency")),
               "tbc_setfull_results_out": (native.SetFullResultsOut, ("outcome", "stable_latency", "lost_latency", "known", "last_present", "last_absent",
                                                                      "summary", "ns_scan", "ns_results", "bytes_scanned", "bytes_matrix"))}
    lines = []
    for name, (_, fields) in structs.items():
        lines.append('printf("%%zu", sizeof(%s));' % name)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in fields]
        lines.append('printf("\\n");')
    lines.append('printf("%u %d %d %d %d %d %d %d\\n", TBC_SETFULL_F_LINEARIZABLE, TBC_SETFULL_NEVER_READ, TBC_SETFULL_STABLE, TBC_SETFULL_LOST,'
                 ' TBC_SETFULL_VALID_FALSE, TBC_SETFULL_VALID_TRUE, TBC_SETFULL_VALID_UNKNOWN, TBC_SETFULL_WORST);')
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tbcheck.h"\nint main(void){ %s return 0; }\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "r.c"), os.path.join(d, "r")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]
    for (name, (S, fields)), row in zip(structs.items(), got):
        assert [f for f, _ in S._fields_] == list(fields), name
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in fields] == row, name
    assert got[3] == [native.SETFULL_F_LINEARIZABLE, native.SETFULL_NEVER_READ, native.SETFULL_STABLE, native.SETFULL_LOST,
                      native.SETFULL_VALID_FALSE, native.SETFULL_VALID_TRUE, native.SETFULL_VALID_UNKNOWN, native.SETFULL_WORST]
    for name in ("tbc_setfull_results", "tbc_setfull_keys_results"):
        assert name in native.SYMBOLS and hasattr(native.lib(), name)
    assert native.lib().tbc_version() == 2


def _host_cases():
    out = []
    for seed in range(6):
        h = set_history(400 + 150 * seed, 4, seed, busy=0.4, info=(0.0, 0.05)[seed % 2], corrupt="lost" if seed % 3 == 0 else None)
        out.append(("plain%d" % seed, h))
        out.append(("timed%d" % seed, _timed(h, seed)))
    out.append(("stale", _timed(_lossy_set_history(3, n_ops=800, lose=0, stale=4)[0], 3)))
    out.append(("adds-only", [o for o in set_history(80, 3, 2) if o["f"] == "add"]))
    out.append(("empty", []))
    for f, h in _edn_setfull_histories().items():
        out.append((f, h))
    return out


def test_result_map_from_device_arrays_equals_the_oracle():
    """`result_from_device` fed with what the device must return (the numpy model over the oracle's three indices) gives the oracle's
    result map, whole: generated histories with and without :time, a lost element, crashed adds, and the EDN goldens."""
    seen = set()
    for name, h in _host_cases():
        enc = sf.Encoded(h)
        assert enc.elements == [e["element"] for e in osf.element_states(h)]
        assert (enc.op_time is None) == (not any("time" in o for o in h))
        for lin in (True, False):
            dev = np_decide(*_states_of(h), enc.op_time, enc.unit, lin)
            got, want = sf.result_from_device(enc, dev), osf.check(h, lin)
            assert got == want, (name, lin)
            seen.add((want["valid?"], bool(want["lost"]), bool(want["stale"]), bool(want["never-read"]), "time" in h[0] if h else None))
    assert {v for v, *_ in seen} == {True, False, "unknown"}
    assert any(s[1] for s in seen) and any(s[2] for s in seen) and any(s[3] for s in seen) and {s[4] for s in seen} >= {True, False}


def test_time_column_is_the_times_of_the_history():
    h = _timed(set_history(300, 3, 5, info=0.05), 5)
    h.insert(10, {"type": "info", "f": "start", "value": None, "process": "nemesis", "time": 1})
    enc = sf.Encoded(h)
    assert enc.unit == MS and enc.op_time.dtype == np.int64 and len(enc.op_time) == enc.n_ops
    assert all(enc.op_time[i] == t for i, t in enc.times.items())
    bare = sf.Encoded(set_history(300, 3, 5))
    assert bare.op_time is None and bare.unit == 1


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_results_have_no_cpu_fallback(native):
    h = set_history(100, 3, 1)
    with pytest.raises(N.NoDeviceError):
        sf.check(h, True)
    with pytest.raises(N.NoDeviceError):
        sf.check_keys({0: h, 1: _timed(h, 1)}, True)
    with pytest.raises(N.NoDeviceError):
        sf.Scan(sf.Encoded(h)).results()


# ---------------------------------------------------------------------------------------------------- GPU tier: inputs
class _Key:
    pass


def _n_ops(a):
    xs = [a.add_invoke, a.add_ok[a.add_ok != NONE], a.read_invoke[:a.R], a.read_ok[:a.R]]
    return max([int(x.max()) for x in xs if len(x)] + [-1]) + 1


def _present(a):
    bits = np.zeros((max(a.R, 1), a.wpr * 32), bool)
    for r in range(a.R):
        bits[r, :int(a.top[r])] = True
        ex = a.exc[int(a.exc_off[r]):int(a.exc_off[r + 1])].astype(np.int64)
        bits[r, ex] ^= True
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint32))


def _all_stable_key(lat):
    """A key whose elements are all stable with exactly the given latencies (unit 1): every add acknowledged, then one read that holds
    everything -- no last-absent, so stable-latency = max(0, 0 - time[add_ok]) and the times are the latencies negated."""
    lat = np.asarray(lat, np.int64)
    E = len(lat)
    a = _Key()
    a.E, a.R, a.wpr = E, 1, max(1, (E + 31) // 32)
    a.add_invoke = (2 * np.arange(E)).astype(np.uint32)
    a.add_ok = a.add_invoke + 1
    a.read_invoke, a.read_ok = np.array([2 * E], np.uint32), np.array([2 * E + 1], np.uint32)
    a.top, a.exc_off, a.exc = np.array([E], np.uint32), np.zeros(2, np.uint64), np.zeros(0, np.uint32)
    t = np.zeros(2 * E + 2, np.int64)
    t[a.add_ok] = -lat
    return a, t


def _late_reads_key(E, R, seed, unread=100):
    """E elements, all but the last `unread` added and acknowledged before R reads that each hold all of those but a few: nearly every
    element is stable, a few are lost (missing from the last read), the late ones never read."""
    rng = np.random.default_rng(seed)
    a = _Key()
    a.E, a.R, a.wpr = E, R, max(1, (E + 31) // 32)
    early = E - unread
    a.add_invoke = np.concatenate([2 * np.arange(early), 2 * early + 2 * R + 2 * np.arange(unread)]).astype(np.uint32)
    a.add_ok = np.where(rng.random(E) < 0.95, a.add_invoke + 1, NONE).astype(np.uint32)
    a.read_invoke = (2 * early + 2 * np.arange(R)).astype(np.uint32)
    a.read_ok = a.read_invoke + 1
    a.top = np.full(R, early, np.uint32)
    holes = [np.sort(rng.choice(early, 5, replace=False)).astype(np.uint32) for _ in range(R)]
    a.exc_off = np.concatenate([[0], np.cumsum([len(x) for x in holes])]).astype(np.uint64)
    a.exc = np.concatenate(holes)
    return a


FAMILIES = ("none", "zero", "equal", "clamped", "huge-ms", "huge-1")


def _family_times(name, n_ops, seed):
    """-> (op_time or None, unit).  zero: one instant, so every latency truncates to 0 ms; equal: time -1 everywhere, unit 1 -- every
    latency is 1 (with a last-absent: (-1 + 1) - (-1); without: 0 - (-1)); clamped: random times, half the differences negative;
    huge: random times in [2^61, 2^62), differences of up to 2^61 ns."""
    rng = np.random.default_rng(seed)
    if name == "none":
        return None, 1
    if name == "zero":
        return np.full(n_ops, 7, np.int64), MS
    if name == "equal":
        return np.full(n_ops, -1, np.int64), 1
    if name == "clamped":
        return rng.integers(-25, 25, n_ops).astype(np.int64), 1
    return rng.integers(2 ** 61, 2 ** 62, n_ops).astype(np.int64), MS if name == "huge-ms" else 1


def _check_family_is_adequate(name, wants):
    """On the reference's answer alone: the family holds what it is there for."""
    sl = np.concatenate([w["stable_latency"][w["outcome"] == N.SETFULL_STABLE] for w in wants])
    ll = np.concatenate([w["lost_latency"][w["outcome"] == N.SETFULL_LOST] for w in wants])
    oc = np.concatenate([w["outcome"] for w in wants])
    assert all((oc == x).any() for x in (N.SETFULL_STABLE, N.SETFULL_LOST, N.SETFULL_NEVER_READ)), name
    if name == "zero":
        assert not sl.any() and not ll.any()
    elif name == "equal":
        assert (sl == 1).all() and len(sl) > 8
    elif name == "clamped":
        assert (sl == 0).any() and (sl > 0).any() and (ll == 0).any() and (ll > 0).any()
    elif name.startswith("huge"):
        assert sl.max() >= 2 ** 33 and ll.max() >= 2 ** 33 and (sl == 0).any()
    else:
        assert (sl > 0).any()


def _keyed_results_equal_numpy(arrs, family, lin, seed=0, ks=None):
    """One keyed object over `arrs`; its results under `family` equal the numpy model over the numpy reduction's three indices."""
    own = ks is None
    ks = ks or sf.KeyedScan(arrs)
    try:
        cols = [_family_times(family, _n_ops(a), seed + i) for i, a in enumerate(arrs)]
        unit = cols[0][1]
        per, tot = ks.results(None if family == "none" else [c[0] for c in cols], unit, lin, indices=True)
        assert len(per) == len(arrs) and tot["ns_results"] > 0
        wants = []
        for i, (a, got, (t, _)) in enumerate(zip(arrs, per, cols)):
            d = _dense_states(a)
            for f in ("known", "last_present", "last_absent"):
                assert np.array_equal(got[f], d[f]), (family, i, a.E, a.R, f)
            want = np_decide(d["known"], d["last_present"], d["last_absent"], t, unit, lin)
            _assert_same(got, want, (family, i, a.E, a.R))
            wants.append(want)
        return per, wants
    finally:
        if own:
            ks.close()


EDGE_E, EDGE_R = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049), (0, 1, 64, 65)


@pytest.fixture(scope="module")
def edge_keys():
    return [_synthetic_key(E, R, 31 * E + R, shuffle_exc=bool((E + R) % 2)) for E in EDGE_E for R in EDGE_R]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_every_edge_shape_in_one_object(native, edge_keys, family):
    _, wants = _keyed_results_equal_numpy(edge_keys, family, True, seed=5)
    _check_family_is_adequate(family, wants)


@pytest.mark.gpu
def test_objects_of_1_3_and_40_keys_with_empty_keys(native):
    mixed = lambda n, seed: [_synthetic_key(E, R, seed + i) for i, (E, R) in enumerate(
        [(0, 3)] + [((7, 300, 65, 2049, 33, 1000)[i % 6], (5, 64, 1, 65, 130)[i % 5]) for i in range(n - 3)] + [(0, 0), (0, 7)])]
    for arrs in ([_synthetic_key(300, 65, 1)], [_synthetic_key(0, 4, 2), _synthetic_key(257, 64, 3), _synthetic_key(0, 0, 4)], mixed(40, 100)):
        arrs = list(arrs)
        if len(arrs) == 40:
            arrs.insert(20, _synthetic_key(0, 9, 77)); arrs.pop(21)          # an empty key in the middle too
            assert arrs[0].E == 0 and arrs[20].E == 0 and arrs[-1].E == 0
        for family, lin in (("clamped", True), ("huge-ms", False)):
            _keyed_results_equal_numpy(arrs, family, lin, seed=9)


@pytest.mark.gpu
def test_a_key_split_across_many_workgroups(native):
    """70,001 elements, 8 reads: 35 workgroups of 2,048 elements count into one key's histograms; beside it a small key.  Every family
    -- `equal` makes 70,001 ties for the eight worst places (the lowest element numbers win) across all of them."""
    arrs = [_late_reads_key(70_001, 8, 4), _synthetic_key(300, 8, 5)]
    assert arrs[0].E > 34 * 2048
    with sf.KeyedScan(arrs) as ks:
        for family in FAMILIES:
            _, wants = _keyed_results_equal_numpy(arrs, family, family != "equal", seed=3, ks=ks)
            if family == "equal":
                assert wants[0]["summary"]["stale_count"] > 60_000
                assert [w["element"] for w in wants[0]["summary"]["worst"]] == sorted(w["element"] for w in wants[0]["summary"]["worst"])
            if family == "huge-1":
                assert wants[0]["summary"]["stable_q"][4] >= 2 ** 60


@pytest.mark.gpu
def test_dense_compact_and_keyed_entry_points_agree(native):
    for E, R, seed in ((1, 1, 1), (33, 65, 2), (257, 64, 3), (2049, 65, 4)):
        a = _synthetic_key(E, R, seed)
        a.present = _present(a)
        t, unit = _family_times("clamped", _n_ops(a), seed)
        d = _dense_states(a)
        want = np_decide(d["known"], d["last_present"], d["last_absent"], t, unit, True)
        with sf.Scan(a, rows=False) as dense, sf.Scan(a, rows=True) as rows, sf.KeyedScan([a]) as keyed:
            for got in (dense.results(t, unit, True), rows.results(t, unit, True), keyed.results([t], unit, True)[0][0]):
                _assert_same(got, want, (E, R))
            _assert_same(dense.results(None, 1, False), np_decide(d["known"], d["last_present"], d["last_absent"], None, 1, False), (E, R, "none"))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 2, 20, 100, 101))
def test_quantile_ranks(native, n):
    rng = np.random.default_rng(n)
    lat = rng.permutation(np.arange(n) * 3 + (rng.integers(0, 2 ** 40) if n > 2 else 0))
    a, t = _all_stable_key(lat)
    with sf.Scan(a, rows=True) as s:
        got = s.results(t, 1, False)
    assert got["summary"]["stable_count"] == n and got["summary"]["lost_q"] is None
    assert got["summary"]["stable_q"] == [osf._quantiles([int(x) for x in lat])[p] for p in (0, 0.5, 0.95, 0.99, 1)]
    assert sorted(got["stable_latency"].tolist()) == sorted(int(x) for x in lat)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("fewer", "exactly", "tie"))
def test_worst_stale(native, case):
    lat = {"fewer": [0, 5, 0, 9, 5, 0, 2],                                         # 4 stale, two equal
           "exactly": [3, 0, 8, 8, 1, 0, 6, 2, 7, 0, 4],                           # 8 stale
           "tie": [7, 9, 0, 7, 3, 9, 7, 9, 1, 9, 7, 9, 7, 0, 9, 3, 7]}[case]       # six 9s, then six 7s for two places: elements 0 and 3
    a, t = _all_stable_key(lat)
    with sf.Scan(a, rows=True) as s:
        got = s.results(t, 1, True)
    want = np_decide(a.add_ok, np.full(a.E, a.read_invoke[0], np.uint32), np.full(a.E, NONE, np.uint32), t, 1, True)
    _assert_same(got, want, case)
    w = got["summary"]["worst"]
    assert len(w) == min(8, sum(1 for x in lat if x > 0))
    if case == "tie":
        assert [x["element"] for x in w] == [1, 5, 7, 9, 11, 14, 0, 3] and [x["latency"] for x in w] == [9] * 6 + [7] * 2


@pytest.mark.gpu
def test_every_verdict_is_reached(native):
    stale_h = _timed(_lossy_set_history(3, n_ops=800, lose=0, stale=4)[0], 3)
    lost_h = _timed(_lossy_set_history(6, n_ops=800, lose=2, stale=0)[0], 6)
    calm, t = _all_stable_key([0] * 40)
    reached = set()
    for h in (stale_h, lost_h):
        for lin in (True, False):
            got, want = sf.check(h, lin), osf.check(h, lin)
            assert got == want
            reached.add((want["valid?"], lin, bool(want["lost"]), bool(want["stale"])))
    assert osf.check(stale_h, True)["stale"] and not osf.check(stale_h, True)["lost"]
    assert (False, True, False, True) in reached and (True, False, False, True) in reached        # stale: false under the flag, true without
    assert any(v is False and lost for v, _, lost, _ in reached)
    with sf.Scan(calm, rows=True) as s:
        assert s.results(t, 1, True)["summary"]["valid"] is True
    only_adds = [o for o in set_history(80, 3, 2) if o["f"] == "add"]
    assert osf.check(only_adds, True)["valid?"] == "unknown" and sf.check(only_adds, True) == osf.check(only_adds, True)
    assert sf.check([], True) == osf.check([], True)


# ---------------------------------------------------------------------------------------------------- GPU tier: end to end
@pytest.mark.gpu
def test_check_check_keys_and_independent_equal_the_oracle(native):
    hists = {}
    for k in range(6):
        h = set_history(700 + 200 * k, 5, 50 + k, busy=0.35, info=0.04, corrupt="lost" if k == 3 else None)
        if k in (1, 4):
            h = _lossy_set_history(50 + k, n_ops=900, lose=2 * (k == 4), stale=4)[0]
        hists[k] = _timed(h, k) if k % 2 == 0 else h
    hists["no-reads"] = [o for o in set_history(120, 3, 98) if o["f"] == "add"]
    wants = {lin: {k: osf.check(h, lin) for k, h in hists.items()} for lin in (True, False)}
    w = wants[True]
    assert any(x["lost"] for x in w.values()) and any(x["stale"] for x in w.values()) and any(x["never-read"] for x in w.values())
    assert any(x["stable-count"] for x in w.values()) and {x["valid?"] for x in w.values()} == {True, False, "unknown"}
    for lin in (True, False):
        assert sf.check_keys(hists, lin) == wants[lin]
        for k in (0, 1, 3):
            assert sf.check(hists[k], lin) == wants[lin][k]
    # independent/checker over the reference's composition: :time is an op's own, so the keyed history keeps each key's
    hist = _keyed(hists, nemesis_every=9, seed=2)
    keys, subs = independent.split(hist)
    subs = {k: [dict(o, index=i) for i, o in enumerate(h)] for k, h in subs.items()}      # (a key's ops numbered within the key, as the encoder numbers them)
    c = independent.checker(jc.compose({"set-full": jc.set_full({"linearizable?": True}), "read-all-invoked-adds": jc.read_all_invoked_adds()}))
    got = c.check({}, hist, {})
    assert list(got["results"]) == keys and set(keys) == set(hists)          # (keys in order of first appearance in the interleaved history)
    for k in keys:
        assert got["results"][k]["set-full"] == osf.check(subs[k], True), k
    two = independent.checker(jc.compose({"a": jc.set_full({"linearizable?": True}), "b": jc.set_full({"linearizable?": False})})).check({}, hist, {})
    for k in keys:
        assert two["results"][k]["a"] == osf.check(subs[k], True) and two["results"][k]["b"] == osf.check(subs[k], False), k


@pytest.mark.gpu
def test_edn_goldens_equal_the_oracle(native):
    hists = _edn_setfull_histories()
    assert len(hists) >= 5
    for lin in (True, False):
        got = sf.check_keys(hists, lin)
        for f, h in hists.items():
            assert got[f] == osf.check(h, lin), (f, lin)
            assert sf.check(h, lin) == got[f], (f, lin)


def _raw_results(handle, fn, n_keys, sumE, op_time=None, time_off=None, unit=1, flags=0, null=None):
    n = max(1, sumE)
    keep = dict(outcome=np.zeros(n, np.uint8), slat=np.zeros(n, np.int64), llat=np.zeros(n, np.int64), summary=(N.SetFullKeySummary * max(1, n_keys))())
    t = N.SetFullTimes()
    if op_time is not None:
        t.op_time, t.time_off = _p(op_time, C.c_int64), _p(time_off, C.c_uint64)
    t.unit, t.flags = unit, flags
    o = N.SetFullResultsOut()
    o.outcome, o.stable_latency, o.lost_latency, o.summary = _p(keep["outcome"], C.c_uint8), _p(keep["slat"], C.c_int64), _p(keep["llat"], C.c_int64), keep["summary"]
    if null == "outcome":
        o.outcome = None
    if null == "summary":
        o.summary = None
    st = getattr(N.lib(), fn)(handle, None if null == "times" else C.byref(t), None if null == "out" else C.byref(o))
    return st, N.lib().tbc_last_error().decode(), keep


@pytest.mark.gpu
def test_input_rules_name_the_entry_point_and_the_key(native):
    arrs = [_synthetic_key(40, 30, s) for s in range(3)]
    lens = [_n_ops(a) for a in arrs]
    sumE = sum(a.E for a in arrs)
    with sf.KeyedScan(arrs) as ks, sf.Scan(arrs[0], rows=True) as one:
        fn = "tbc_setfull_keys_results"
        off = lambda ls: np.concatenate([[0], np.cumsum(ls)]).astype(np.uint64)
        ok_t = np.zeros(sum(lens), np.int64)
        assert _raw_results(ks._h, fn, 3, sumE, ok_t, off(lens))[0] == 0
        short = list(lens); short[1] -= 1
        st, msg, _ = _raw_results(ks._h, fn, 3, sumE, ok_t, off(short))
        assert st == N.ERR_INVALID_ARG and fn in msg and "key 1" in msg, msg
        st, msg, _ = _raw_results(ks._h, fn, 3, sumE, ok_t, off(lens), unit=0)
        assert st == N.ERR_INVALID_ARG and fn in msg and "unit" in msg, msg
        for null in ("times", "out", "outcome", "summary"):
            st, msg, _ = _raw_results(ks._h, fn, 3, sumE, ok_t, off(lens), null=null)
            assert st == N.ERR_INVALID_ARG and fn in msg and "null" in msg, (null, msg)
        st, msg, _ = _raw_results(None, fn, 3, sumE, ok_t, off(lens))
        assert st == N.ERR_INVALID_ARG and fn in msg
        st, msg, _ = _raw_results(one._h, "tbc_setfull_results", 1, arrs[0].E, ok_t, off([lens[0] - 1]))
        assert st == N.ERR_INVALID_ARG and "tbc_setfull_results" in msg and "key 0" in msg, msg
        # a longer slice than needed is fine; the object still works after the refusals
        assert _raw_results(one._h, "tbc_setfull_results", 1, arrs[0].E, np.zeros(lens[0] + 5, np.int64), off([lens[0] + 5]))[0] == 0


@pytest.mark.gpu
def test_reruns_threads_and_run_after_results(native):
    a = [_synthetic_key(E, R, 400 + E) for E, R in ((2049, 65), (33, 64), (0, 3), (5000, 40))]
    b = [sf.Encoded(_timed(set_history(1500, 5, 300 + k, busy=0.3), k)) for k in range(4)]
    ta = [_family_times("clamped", _n_ops(x), i)[0] for i, x in enumerate(a)]
    tb = [e.op_time for e in b]
    blob = lambda per: b"".join(p[f].tobytes() for p in per for f in ("outcome", "stable_latency", "lost_latency")) + repr([p["summary"] for p in per]).encode()
    with sf.KeyedScan(a) as ka, sf.KeyedScan(b) as kb:
        before = ka.run()[0]
        first = [blob(ka.results(ta, 1, True)[0]), blob(kb.results(tb, MS, True)[0])]
        assert blob(ka.results(ta, 1, True)[0]) == first[0] and blob(kb.results(tb, MS, True)[0]) == first[1]
        # the raw bytes of a call, summaries' padding and all
        raw = [_raw_results(ka._h, "tbc_setfull_keys_results", len(a), int(ka.Es.sum()), np.concatenate(ta),
                            np.concatenate([[0], np.cumsum([len(t) for t in ta])]).astype(np.uint64))[2] for _ in range(2)]
        assert all(bytes(raw[0][f]) == bytes(raw[1][f]) for f in ("outcome", "slat", "llat", "summary"))
        res = [[], []]
        th = [threading.Thread(target=lambda i=i, o=o, t=t, u=u: [res[i].append(blob(o.results(t, u, True)[0])) for _ in range(4)])
              for i, (o, t, u) in enumerate(((ka, ta, 1), (kb, tb, MS)))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert res[0] == [first[0]] * 4 and res[1] == [first[1]] * 4
        after = ka.run()[0]
        for x, y, k in zip(before, after, a):
            d = _dense_states(k)
            for f in ("known", "last_present", "last_absent"):
                assert np.array_equal(x[f], y[f]) and np.array_equal(y[f], d[f])
        # a call with other times (and none) on the same object
        assert blob(ka.results(None, 1, False)[0]) != first[0]
        assert blob(ka.results(ta, 1, True)[0]) == first[0]

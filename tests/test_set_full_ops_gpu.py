"""The history as op columns on the GPU (tbc_setfull_keys_create_ops: csrc/set_full_encode_plan.h plans, csrc/set_full_encode.h's kernels
build the matrix from the reads' raw values): an object made from ops gives what an object made from `Encoded`'s compact form of the same
histories gives -- the three indices, outcomes, latencies, summaries -- and its encoding is `Encoded`'s; `check_keys_columns` returns
`check_keys`' result maps, the EDN goldens included.  No malformed input here: that is refused on the host (tests/test_set_full_ops.py)."""
import json
import os
import threading

import numpy as np
import pytest

from helpers import GOLDEN, set_history
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import edn, set_full as sf
from test_set_full_encode_emu import HAND, _h, assert_equals_encoded, shape_history

pytestmark = pytest.mark.gpu
WINDOW = 32 * N.SETFULL_ENCODE_WINDOW_WORDS          # the values kernel's window, in elements


def _per_key(enc):
    ce = np.concatenate([[0], np.cumsum(enc["n_elements"], dtype=np.int64)])
    cr = np.concatenate([[0], np.cumsum(enc["n_reads"], dtype=np.int64)])
    out = []
    for k in range(len(enc["n_elements"])):
        d = {f: enc[f][ce[k]:ce[k + 1]] for f in ("element", "add_invoke", "add_ok", "dup_max")}
        d.update({f: enc[f][cr[k]:cr[k + 1]] for f in ("read_invoke", "read_ok")})
        d.update(dup_count=int(enc["dup_count"][k]), unknown_values=int(enc["unknown_values"][k]))
        out.append(d)
    return out


def _times(objs):
    return None if all(o is None for o, _ in objs) else [t if t is not None else np.arange(n, dtype=np.int64) for t, n in objs]


def _assert_from_ops_equals_encoded(hists, unit=1, lin=True):
    """-> the per-key encoding.  from_ops(columns) against KeyedScan([Encoded ...]) on the same histories: run(), results(), encoding()."""
    cols = sf.OpColumns.of_keys(hists)
    encs = [sf.Encoded(h) for h in hists.values()]
    with sf.KeyedScan.from_ops(cols) as ko, sf.KeyedScan(encs) as ke:
        assert ko.shape() == ke.shape() == (sum(e.E for e in encs), sum(e.R for e in encs))
        assert np.array_equal(ko.Es, ke.Es) and np.array_equal(ko.Rs, ke.Rs)
        enc = ko.encoding()
        per_o, tot_o = ko.run()
        per_e, tot_e = ke.run()
        assert tot_o["bytes_matrix"] == tot_e["bytes_matrix"] and tot_o["bytes_scanned"] == tot_e["bytes_scanned"]
        res_o, _ = ko.results(_times(list(zip(cols.op_time, cols.n_ops))), unit, lin, indices=True)
        res_e, _ = ke.results(_times([(e.op_time, e.n_ops) for e in encs]), unit, lin, indices=True)
        with pytest.raises(N.TbcError, match="not made from ops"):
            ke.encoding()
    got = _per_key(enc)
    for k, (name, h) in enumerate(hists.items()):
        assert_equals_encoded(got[k], h, name)
        for f in ("known", "last_present", "last_absent"):
            assert np.array_equal(per_o[k][f], per_e[k][f]), (name, f)
            assert np.array_equal(res_o[k][f], res_e[k][f]), (name, f)
        for f in ("outcome", "stable_latency", "lost_latency"):
            assert np.array_equal(res_o[k][f], res_e[k][f]), (name, f)
        assert res_o[k]["summary"] == res_e[k]["summary"], name
    return got, enc


def test_from_ops_equals_encoded_on_histories():
    hists = {k: set_history(1500 + 400 * k, 6, 300 + k, busy=0.3, info=0.05, corrupt=c) for k, c in enumerate((None, "lost", "phantom", None))}
    hists[3] = [dict(o, time=1_000_000 * i + 17) for i, o in enumerate(hists[3])]
    got, enc = _assert_from_ops_equals_encoded({k: hists[k] for k in (0, 1, 2)})
    assert enc["ns_encode"] > 0 and got[2]["unknown_values"] == 1 and not enc["dup_max"].any()
    _assert_from_ops_equals_encoded({3: hists[3]}, unit=1_000_000)


def test_edge_shapes_and_hand_cases():
    """The shapes and hand cases of the emulator test, in one object: E in {0, 1, 31, 33, 64, 65, 257} x R in {0, 1, 64, 65}, empty keys
    first, in the middle and last."""
    hists = {"first": []}
    for E in (0, 1, 31, 33, 64, 65, 257):
        for R in (0, 1, 64, 65):
            hists[(E, R)] = shape_history(E, R, 100 * E + R, unknown=2 if (E + R) % 2 else 0)
        if E == 33:
            hists["middle"] = []
    hists.update(HAND)
    hists["last"] = []
    got, enc = _assert_from_ops_equals_encoded(hists)
    assert not enc["dup_max"].any() and not enc["dup_count"].any()
    assert sf.check_keys_columns(hists, True) == sf.check_keys(hists, True)


def test_256_keys_in_one_object():
    hists = {k: set_history(200, 4, 1000 + k, busy=0.4, info=0.03, corrupt=("lost", "phantom", None, None)[k % 4]) for k in range(256)}
    _assert_from_ops_equals_encoded(hists)
    assert sf.check_keys_columns(hists, True) == sf.check_keys(hists, True)


def test_a_row_wider_than_the_window():
    """One key of 3 reads over window + 70 elements: the second pass over each read's values runs and keeps the last 70 columns."""
    E = WINDOW + 70
    adds = [op for v in range(E) for op in (("invoke", "add", v, 0), ("ok", "add", v, 0))]
    rng = np.random.default_rng(5)
    full = rng.permutation(E)
    reads = [full[full % 3 != 0].tolist(), [E - 1, 0, WINDOW, WINDOW - 1, E - 35, 12345], full.tolist()]
    h = _h(adds + [op for r in reads for op in (("invoke", "read", None, 1), ("ok", "read", r, 1))])
    cols = sf.OpColumns(h)
    with sf.KeyedScan.from_ops(cols) as ko:
        assert ko.shape() == (E, 3)
        per, _ = ko.run()
        enc = ko.encoding()
    assert enc["element"].tolist() == list(range(E)) and not enc["dup_max"].any() and enc["unknown_values"][0] == 0
    inv = [2 * E, 2 * E + 2, 2 * E + 4]
    # every element was added before every read: last_present / last_absent say which reads held it, column by column
    e = np.arange(E)
    small = np.isin(e, reads[1])
    lp = np.full(E, inv[2])
    la = np.where(small, np.where(e % 3 == 0, inv[0], N.NO_OP), inv[1])
    assert np.array_equal(per[0]["last_present"], lp) and np.array_equal(per[0]["last_absent"], la.astype(np.uint32))
    assert np.array_equal(per[0]["known"], (2 * e + 1).astype(np.uint32))


def test_duplicates_run_the_dups_kernel_and_their_absence_does_not():
    dup = {"two-and-three": shape_history(40, 6, 1, dup=((2, 3, 2), (4, 3, 3))),
           "clean": shape_history(70, 5, 2, unknown=1),
           "wide": shape_history(600, 4, 3, dup=((3, 10, 2), (3, 300, 3), (3, 590, 2))),
           "unknown-dup": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", [8, 1, 8, 8], 1)]),
           "both": _h([("invoke", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", [60, 1, 1, 60, 50, 60], 1)])}
    got, enc = _assert_from_ops_equals_encoded(dup)
    assert enc["dup_count"].tolist() == [1, 0, 3, 0, 1] and enc["unknown_values"].tolist()[3:] == [3, 4]
    res = sf.check_keys_columns(dup, False)
    assert res == sf.check_keys(dup, False)
    assert res["unknown-dup"]["duplicated"] == {8: 3} and res["both"]["duplicated"] == {1: 2, 60: 3} and res["both"]["valid?"] is False
    assert res["clean"]["duplicated"] == {} and res["two-and-three"]["duplicated-count"] == 1
    clean = {k: dup[k] for k in ("clean",)}
    got, enc = _assert_from_ops_equals_encoded(clean)
    assert not enc["dup_max"].any() and not enc["dup_count"].any()


def test_check_keys_columns_on_the_edn_goldens():
    d = os.path.join(GOLDEN, "edn_checkers")
    cases = [c for c in json.load(open(os.path.join(d, "expected.json")))["cases"] if c["checker"] == "set-full"]
    files = sorted({c["file"] for c in cases})
    hists = {f: edn.read_history(os.path.join(d, f)) for f in files}
    keys = ("valid?", "attempt-count", "stable-count", "lost-count", "lost", "never-read-count", "never-read", "stale-count", "stale", "duplicated-count")
    for lin in (True, False):
        got = sf.check_keys_columns(hists, lin)
        assert got == sf.check_keys(hists, lin)
        seen = 0
        for case in cases:
            if case["opts"]["linearizable?"] is not lin:
                continue
            r = got[case["file"]]
            for k in keys:
                assert r[k] == case["expect"][k], (case["file"], lin, k)
            assert {str(k): v for k, v in r["duplicated"].items()} == case["expect"]["duplicated"]
            seen += 1
        assert seen >= 6
    for f in files:
        assert sf.check_columns(hists[f], True) == sf.check(hists[f], True), f


def test_forced_budget_split(monkeypatch):
    hists = {k: set_history(600 + 150 * k, 5, 70 + k, busy=0.3, corrupt="phantom" if k == 3 else None) for k in range(7)}
    hists[5] = [dict(o, time=1_000_000 * i) for i, o in enumerate(hists[5])]          # (a latency unit of its own: a call of its own)
    whole = sf.check_keys_columns(hists, True)
    assert whole == sf.check_keys(hists, True) and list(whole) == list(hists)
    calls = []
    real = sf.KeyedScan.from_ops.__func__

    def counting(cls, columns, device=0):
        calls.append(list(columns.keys))
        return real(cls, columns, device)

    monkeypatch.setattr(sf.KeyedScan, "from_ops", classmethod(counting))
    cols = sf.OpColumns.of_keys(hists)
    monkeypatch.setattr(sf, "KEYS_BUDGET_BYTES", max(sf._matrix_bytes(sf._Bound(a, r)) for a, r in zip(cols.n_add_invokes, cols.n_ok_reads)))
    assert sf.check_keys_columns(hists, True) == whole
    assert len(calls) >= 3 and sorted(k for c in calls for k in c) == list(range(7)) and [5] in calls


def test_two_objects_from_two_threads():
    a = {k: set_history(800, 5, 400 + k, busy=0.3, info=0.02) for k in range(6)}
    b = {k: shape_history(E, R, E + R, unknown=1) for k, (E, R) in enumerate(((257, 65), (33, 64), (0, 5), (600, 9)))}
    want = [sf.check_keys(a, True), sf.check_keys(b, True)]
    res = [[], []]
    th = [threading.Thread(target=lambda i=i, h=h: [res[i].append(sf.check_keys_columns(h, True)) for _ in range(3)]) for i, h in enumerate((a, b))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert len(res[0]) == len(res[1]) == 3
    assert all(r == want[0] for r in res[0]) and all(r == want[1] for r in res[1])

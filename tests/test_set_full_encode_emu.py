"""tbc_setfull_keys_create_ops's encoding on the CPU: the host plan (csrc/set_full_encode_plan.h) and the encoding kernels
(csrc/set_full_encode.h, the file hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator of tests/emu
(tests/emu/emu_setfull_encode.cpp runs plan -> table build -> values kernel -> dups kernel in the library's order, with a window of 8
words = 256 elements), against jepsen/set_full.py `Encoded` of the same histories: elements and the four index columns, the matrix --
every word of every pitch -- the duplicates and the unknown values, exactly, under two seeded interleavings of the wavefronts.  Test
infrastructure only: the product has no CPU path."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import set_history
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.columns import _p
from jepsen_tigerbeetle_amd.jepsen import set_full as sf

SEEDS = (1, 2)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_sfe") / "libemu_sfe.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_setfull_encode.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.emu_sfe_encode.restype = C.c_int
    lib.emu_sfe_error.restype = C.c_char_p
    lib.emu_sfe_window_words.restype = C.c_uint32
    return lib


def ops_in(cols, device=0):
    """A tbc_setfull_ops_in over an OpColumns (and the arrays it points into)."""
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    keep = {f: pad(getattr(cols, f)) for f in ("op_off", "index", "type", "f", "process", "value", "val_off", "vals")}
    s = N.SetFullOpsIn()
    s.n_keys, s.device = len(cols.keys), device
    s.op_off, s.val_off = _p(keep["op_off"], C.c_uint64), _p(keep["val_off"], C.c_uint64)
    s.index, s.type, s.f = _p(keep["index"], C.c_uint32), _p(keep["type"], C.c_uint8), _p(keep["f"], C.c_uint8)
    s.process, s.value, s.vals = _p(keep["process"], C.c_int64), _p(keep["value"], C.c_int64), _p(keep["vals"], C.c_int64)
    return s, keep


def emu_encode(lib, hists, seed, grid=3):
    """-> per key {"element", "add_invoke", ..., "dup_max", "dup_count", "unknown_values", "M" (R x PITCH words)}, and the totals"""
    cols = sf.OpColumns.of_keys(hists)
    s, keep = ops_in(cols)
    rc = lib.emu_sfe_encode(C.byref(s), C.c_uint32(grid), C.c_uint64(seed))
    assert rc == 0, lib.emu_sfe_error().decode()
    shape = (C.c_uint64 * 5)()
    lib.emu_sfe_shape(shape)
    sumE, sumR, m_words, repeats, dups_ran = (int(x) for x in shape)
    n = len(cols.keys)
    z = lambda m, dt: np.zeros(max(1, m), dt)
    a = {"n_elements": z(n, np.uint32), "n_reads": z(n, np.uint32), "element": z(sumE, np.int64), "add_invoke": z(sumE, np.uint32),
         "add_ok": z(sumE, np.uint32), "read_invoke": z(sumR, np.uint32), "read_ok": z(sumR, np.uint32), "dup_max": z(sumE, np.uint32),
         "dup_count": z(n, np.uint32), "unknown_values": z(n, np.uint64)}
    e = N.SetFullEncoding()
    ct = {np.dtype(np.uint32): C.c_uint32, np.dtype(np.int64): C.c_int64, np.dtype(np.uint64): C.c_uint64}
    for f, x in a.items():
        setattr(e, f, _p(x, ct[x.dtype]))
    pitch, m_off, M = z(n, np.uint32), z(n, np.uint64), z(m_words, np.uint32)
    lib.emu_sfe_get(C.byref(e), _p(pitch, C.c_uint32), _p(m_off, C.c_uint64), _p(M, C.c_uint32))
    ce = np.concatenate([[0], np.cumsum(a["n_elements"][:n], dtype=np.int64)])
    cr = np.concatenate([[0], np.cumsum(a["n_reads"][:n], dtype=np.int64)])
    per = []
    for k in range(n):
        E, R, P = int(a["n_elements"][k]), int(a["n_reads"][k]), int(pitch[k])
        d = {f: a[f][ce[k]:ce[k + 1]] for f in ("element", "add_invoke", "add_ok", "dup_max")}
        d.update({f: a[f][cr[k]:cr[k + 1]] for f in ("read_invoke", "read_ok")})
        d.update(dup_count=int(a["dup_count"][k]), unknown_values=int(a["unknown_values"][k]), E=E, R=R, PITCH=P,
                 M=M[int(m_off[k]):int(m_off[k]) + R * P].reshape(R, P))
        per.append(d)
    return per, {"repeats": repeats, "dups_ran": dups_ran}


def assert_equals_encoded(got, history, ctx):
    """one key of the emulator's (or the library's) encoding against `Encoded` of its history"""
    enc = sf.Encoded(history)
    assert got["element"].tolist() == enc.elements, ctx
    for f in ("add_invoke", "add_ok", "read_invoke", "read_ok"):
        assert np.array_equal(got[f], getattr(enc, f)), (ctx, f)
    if "M" in got:
        assert got["PITCH"] == ((enc.E + 31) // 32 + 3) // 4 * 4, ctx
        want = np.zeros((enc.R, got["PITCH"]), np.uint32)
        if enc.E and enc.R:
            want[:, :enc.wpr] = enc.present[:enc.R]
        assert np.array_equal(got["M"], want), ctx
    names = set(enc.elements)
    dups = {int(v): int(m) for v, m in zip(got["element"], got["dup_max"]) if m > 1}
    assert dups == {v: m for v, m in enc.duplicated.items() if v in names}, ctx
    assert all(m == 0 or m > 1 for m in got["dup_max"]), ctx
    assert got["dup_count"] == len(dups), ctx
    hist = list(history)
    unknown = sum(sum(1 for x in hist[int(i)]["value"] if x not in names) for i in enc.read_ok)
    assert got["unknown_values"] == unknown, ctx
    return enc


def shape_history(E, R, seed, dup=(), unknown=0, shuffle=True):
    """E adds and R reads on one timeline: a read returns a random subset of the elements invoked so far (a tenth of them left out),
    shuffled; dup = ((read number, element position, multiplicity), ...) repeats that element in that read, the copies spread over the
    value; unknown: that many values nobody added in every third read."""
    rng = random.Random(seed)
    kinds = ["add"] * E + ["read"] * R
    rng.shuffle(kinds)
    if R:                                                  # (a last read that sees everything)
        kinds.remove("read"); kinds.append("read")
    h, added, n_read = [], [], 0
    for kind in kinds:
        if kind == "add":
            v = 1000 + 7 * len(added)
            added.append(v)
            h.append({"type": "invoke", "f": "add", "value": v, "process": 0})
            h.append({"type": "ok" if rng.random() < 0.9 else "info", "f": "add", "value": v, "process": 0})
        else:
            vals = [v for v in added if rng.random() < 0.9] if n_read < R - 1 else list(added)
            for rd, pos, mult in dup:
                if rd == n_read and pos < len(added):
                    vals = [v for v in vals if v != added[pos]] + [added[pos]] * mult
            if unknown and n_read % 3 == 0:
                vals += [5 + i for i in range(unknown)]
            if shuffle:
                rng.shuffle(vals)
            for rd, pos, mult in dup:                      # (the first and the last value: two strides of the workgroup apart where they can be)
                if rd == n_read and pos < len(added) and mult == 2:
                    vals = [added[pos]] + [v for v in vals if v != added[pos]] + [added[pos]]
            p = 1 + n_read % 3
            h.append({"type": "invoke", "f": "read", "value": None, "process": p})
            h.append({"type": "ok", "f": "read", "value": vals, "process": p})
            n_read += 1
    return [dict(o, index=i) for i, o in enumerate(h)]


def _h(rows):
    return [{"type": t, "f": f, "value": v, "process": p, "index": i} for i, (t, f, v, p) in enumerate(rows)]


HAND = {
    "re-added": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "add", 2, 0), ("ok", "add", 2, 0), ("invoke", "read", None, 1),
                    ("ok", "read", [1, 2], 1), ("invoke", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", [2], 1), ("ok", "add", 1, 0),
                    ("invoke", "read", None, 2), ("ok", "read", [2, 1], 2)]),
    "ok-before-re-invocation": _h([("invoke", "add", 5, 0), ("ok", "add", 5, 0), ("invoke", "add", 5, 1), ("invoke", "read", None, 2),
                                   ("ok", "read", [5], 2), ("invoke", "add", 6, 0), ("ok", "add", 6, 3), ("ok", "add", 6, 0), ("ok", "add", 9, 0)]),
    "fail-read": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "read", None, 1), ("fail", "read", None, 1), ("ok", "read", [1], 1),
                     ("invoke", "read", None, 1), ("ok", "read", [1], 1)]),
    "info-read-then-invoke": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "read", None, 1), ("info", "read", None, 1),
                                 ("invoke", "add", 2, 0), ("invoke", "read", None, 1), ("ok", "read", [1, 2], 1), ("invoke", "read", None, 2),
                                 ("info", "read", None, 2), ("ok", "read", [1], 2)]),
    "nil-read": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", None, 1), ("ok", "read", [1], 1),
                    ("invoke", "read", None, 1), ("ok", "read", [1], 1)]),
    "empty-read": _h([("invoke", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", [], 1), ("ok", "add", 1, 0), ("invoke", "read", None, 1),
                      ("ok", "read", [1], 1)]),
    "ok-read-without-invocation": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("ok", "read", [1, 1], 4), ("invoke", "read", None, 1),
                                      ("ok", "read", [], 1), ("invoke", "read", None, 2), ("ok", "read", [1, 77, 77], 2)]),
}


def test_hand_cases_equal_encoded(emu):
    assert emu.emu_sfe_window_words() == 8
    for seed in SEEDS:
        per, _ = emu_encode(emu, HAND, seed)
        for (name, h), got in zip(HAND.items(), per):
            assert_equals_encoded(got, h, (name, seed))
    # what the cases are there for
    per, _ = emu_encode(emu, HAND, 1)
    by = dict(zip(HAND, per))
    assert by["re-added"]["element"].tolist() == [2, 1] and by["re-added"]["add_invoke"].tolist() == [2, 6] and by["re-added"]["add_ok"].tolist() == [3, 9]
    assert by["ok-before-re-invocation"]["add_ok"].tolist() == [N.NO_OP, 6]
    assert by["fail-read"]["R"] == 1 and by["info-read-then-invoke"]["read_invoke"].tolist() == [5, 7]
    assert by["nil-read"]["R"] == 1 and by["empty-read"]["R"] == 2 and not by["empty-read"]["M"][0].any()
    assert by["ok-read-without-invocation"]["R"] == 2 and by["ok-read-without-invocation"]["unknown_values"] == 2


@pytest.mark.parametrize("corrupt", (None, "lost", "phantom"))
def test_generated_histories_equal_encoded(emu, corrupt):
    hists = {k: set_history(n, 4, 20 + k, busy=0.4, info=0.1, corrupt=corrupt) for k, n in enumerate((300, 0, 120, 700))}
    assert any(o["type"] == "info" for o in hists[0])
    for seed in SEEDS:
        per, tot = emu_encode(emu, hists, seed)
        for k, got in enumerate(per):
            assert_equals_encoded(got, hists[k], (corrupt, k, seed))
        assert tot["dups_ran"] == 0 and all(not g["dup_max"].any() for g in per)
        assert (sum(g["unknown_values"] for g in per) > 0) == (corrupt == "phantom")


def test_edge_shapes_equal_encoded(emu):
    """E in {0, 1, 31, 33, 64, 65, 257} x R in {0, 1, 64, 65} (64: a table of exactly 2 E slots; 257: two windows), an empty key first,
    in the middle and last, one key of three windows; read values shuffled; unknown values in some keys."""
    hists = {"first": []}
    for E in (0, 1, 31, 33, 64, 65, 257):
        for R in (0, 1, 64, 65):
            hists[(E, R)] = shape_history(E, R, 100 * E + R, unknown=2 if (E + R) % 2 else 0)
        if E == 33:
            hists["middle"] = []
    hists["three-windows"] = shape_history(520, 3, 9)
    hists["last"] = []
    for seed in SEEDS:
        per, tot = emu_encode(emu, hists, seed, grid=5)
        for (name, h), got in zip(hists.items(), per):
            assert_equals_encoded(got, h, (name, seed))
        assert tot["repeats"] == 0 and tot["dups_ran"] == 0
    by = dict(zip(hists, per))
    assert by[(257, 64)]["PITCH"] == 12 and by["three-windows"]["PITCH"] == 20 and by[(64, 1)]["PITCH"] == 4
    assert by[(0, 65)]["R"] == 65 and by[(0, 65)]["PITCH"] == 0 and by[(0, 65)]["unknown_values"] > 0


def test_duplicates(emu):
    """Multiplicity 2 and 3 of one element in different reads (the greater counts); repeats in columns of different windows of one row,
    found in different passes over its values, the two copies of a pair a whole read apart; a key without repeats next to them keeps
    dup_max all zero; duplicated unknown values are counted as unknown and nothing else."""
    hists = {"two-and-three": shape_history(40, 6, 1, dup=((2, 3, 2), (4, 3, 3))),
             "clean": shape_history(70, 5, 2, unknown=1),
             "windows": shape_history(600, 4, 3, dup=((3, 10, 2), (3, 300, 3), (3, 590, 2))),
             "unknown-dup": _h([("invoke", "add", 1, 0), ("ok", "add", 1, 0), ("invoke", "read", None, 1), ("ok", "read", [8, 1, 8, 8], 1)])}
    for seed in SEEDS:
        per, tot = emu_encode(emu, hists, seed)
        encs = {name: assert_equals_encoded(got, h, (name, seed)) for (name, h), got in zip(hists.items(), per)}
        assert tot["dups_ran"] == 1 and tot["repeats"] >= 7
    by = dict(zip(hists, per))
    assert sorted(by["two-and-three"]["dup_max"].tolist())[-2:] == [0, 3] and by["two-and-three"]["dup_count"] == 1
    assert not by["clean"]["dup_max"].any() and by["clean"]["dup_count"] == 0
    assert by["windows"]["dup_count"] == 3 and sorted(m for m in by["windows"]["dup_max"].tolist() if m) == [2, 2, 3]
    assert [int(e) // 256 for e in np.nonzero(by["windows"]["dup_max"])[0]] == [0, 1, 2]          # (a window is 256 elements)
    assert by["unknown-dup"]["dup_count"] == 0 and by["unknown-dup"]["unknown_values"] == 3 and encs["unknown-dup"].duplicated == {8: 3}


def test_bad_columns_are_refused_by_the_plan(emu):
    cols = sf.OpColumns.of_keys({0: HAND["re-added"], 1: HAND["fail-read"]})
    s, keep = ops_in(cols)
    keep["f"][3] = 7
    assert emu.emu_sfe_encode(C.byref(s), C.c_uint32(1), C.c_uint64(1)) == 1
    assert "key 0 op 3" in emu.emu_sfe_error().decode()

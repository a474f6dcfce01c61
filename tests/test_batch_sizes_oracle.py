"""The histories of tests/test_batch_sizes_gpu.py (tests/batch_size_shapes.py) WITHOUT a GPU: every family has the shape it is named for, the
oracle decides every base history (none skipped, none unknown, a third invalid), a batch puts different base histories on both sides of
every class edge, a fresh input fits the batch it is sent to, and the place where the lists outgrow the arena splits a thread's run."""
import numpy as np
import pytest

import batch_size_shapes as S
from jepsen_tigerbeetle_amd import _native as N


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_the_oracle_decides_every_base_history_of_a_family(native, oracle, name):
    for which in ("base", "other"):
        refs = S.references(oracle, name, which)
        assert len(refs) == S.N_BASE
        hists = S.base(name) if which == "base" else S.other_base(name)
        assert len({(len(h), h.n_events, bytes(np.asarray(h.a))) for h in hists}) == S.N_BASE          # 61 distinct histories
        assert len({len(h) % 4 for h in hists}) == 4
        # a history answered with a neighbour's result would show: no two neighbours share verdict, failing op and counters
        what = [(r["valid"], r["fail_op"], r["probes"], r["visited"], r["backtracks"]) for r in refs]
        assert all(what[j] != what[(j + 1) % S.N_BASE] for j in range(S.N_BASE)) and len(set(what)) >= S.N_BASE - 3
        for r, h in zip(refs, hists):
            if r["valid"] == 0:
                assert 0 <= r["fail_op"] < len(h)
            if S.FAMILIES[name].kind == "count":
                assert r["how"] == "exact" and r["probes"] < S.budget_of([min(hists, key=len)])       # (no batch's budget bites: one reference serves every size)


def test_both_sides_of_every_class_edge_hold_different_histories(native):
    for n in S.SIZES + (S.OVERFLOW_N,):
        idx = S.indices(n)
        assert len(idx) == n and all(0 <= j < S.N_BASE for j in idx)
        for edge in S.EDGES:
            if n > edge:
                assert idx[edge - 1] != idx[edge] and idx[edge] != idx[0] and idx[edge - 1] != idx[n - 1], (n, edge)
        if n >= S.N_BASE:
            assert set(idx) == set(range(S.N_BASE))
    assert len({S.indices(n)[0] for n in S.SIZES}) > len(S.SIZES) // 2                                  # the sizes start at different histories
    for name in ("long-neighbour-wide", "long-neighbour-narrow"):
        for n in S.LONG_SIZES:
            b = S.batch_of(name, n)
            assert [i for i, h in enumerate(b) if len(h) > S.GEO_OPS] == [n // 2]


def test_a_fresh_input_fits_the_batch_it_is_sent_to(native):
    cases = S.reload_cases()
    assert {t for _, _, _, t in cases} == {0, 1, 2, 3}
    for name in S.STREAM_FAMILIES:
        assert {t for nm, _, _, t in cases if nm == name} == {0, 1, 2, 3}, name
    for name, nc, nr, t in cases:
        first, _, (nxt, idx, which) = S.reload_plan(name, nc, nr, t)
        assert (len(first), len(nxt)) == (nc, nr)
        t_first, t_next = sum(len(h) for h in first), sum(len(h) for h in nxt)
        assert t_next % 4 == t and t_next <= t_first + t_first // 8, (name, nc, nr)
        assert S.mask_words(nxt) <= S.mask_words(first), (name, nc, nr)
        if S.FAMILIES[name].long_neighbour:               # the history that sends the whole batch to pack_kernel: created with one, reloaded with one
            assert first[nc // 2] is S.long_neighbour() and nxt[nr // 2] is S.long_neighbour()
        if S.largest_value(first) <= 30:                  # (a batch with rule tables takes no value beyond its first input's)
            assert S.largest_value(nxt) <= S.largest_value(first), (name, nc, nr)
        if nr > 3:
            assert any(which) and not all(which) and sum(x is not y for x, y in zip(nxt, first)) > nr // 2


def test_the_lists_outgrow_the_arena_in_the_middle_of_a_threads_run(native):
    quiet, dense, _ = S.overflow_batches()
    per = (S.OVERFLOW_N + 1023) // 1024
    start = S.fallback_start(quiet, dense)
    assert per == 2 and 0 < start < S.OVERFLOW_N and start % per != 0, start
    assert S.fallback_start(dense, dense) == S.OVERFLOW_N                                                # (and once the arena has grown, everything fits)
    # the count is the definition's: every front's open calls, one by one
    h = dense[0]
    inv, ret, f = (np.asarray(x).astype(np.int64) for x in (h.inv_pos, h.ret_pos, h.f))
    total = sum(1 for r in ret for i in range(len(h)) if f[i] != N.F_READ and inv[i] < r and ret[i] >= r)
    assert S.list_entries(h) == total


def test_the_wire_edge_input_holds_254_in_both_paths(native):
    hists = S.wire_edge_input()
    f, a, b = (np.concatenate([np.asarray(getattr(h, k)) for h in hists]) for k in ("f", "a", "b"))
    T = len(f)
    assert T % 4 == 3
    vec, tail = slice(0, T - 3), slice(T - 3, T)
    for part in (vec, tail):
        assert ((f[part] == N.F_WRITE) & (a[part] == 254)).any() and ((f[part] == N.F_CAS) & (a[part] == 254)).any() and ((f[part] == N.F_CAS) & (b[part] == 254)).any()
        assert ((f[part] == N.F_READ) & (a[part] == N.NIL)).any()
    assert int(a[a != N.NIL].max()) == 254 and int(a[a != N.NIL].min()) >= 0

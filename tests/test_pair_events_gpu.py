"""tbc_pair_events_batch on the MI355X: the shapes of tests/pair_events_shapes.py through the entry point, every array bit for bit what
tbc_pair_events gives history by history (descriptors, the six op columns, the wire word, status and bad row), the capacity rule, and
core.Batch.reload_events -- event histories paired on the device into a mapped input slot and submitted -- answered exactly as
Batch.reload of the host-paired columns: verdict, failing op, every counter, on a crash-free batch and on count-form batches of both
kernels (chosen as tests/test_stream_gpu.py chooses them)."""
import ctypes as C

import numpy as np
import pytest

import pair_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns, core, synth

pytestmark = pytest.mark.gpu

CASES = sorted(S.cases())
KEYS = ("valid", "fail_op", "prev_ok_op", "probes", "visited", "backtracks", "max_depth", "steps", "final_state")


def run(evs, word=False, ops_cap=None, columns_wanted=True):
    ev_off, ev = columns.concat_events(evs)
    return columns.pair_events_batch_raw(ev_off, ev, ops_cap=ops_cap, word=word, columns=columns_wanted)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_tbc_pair_events(native, name):
    evs = S.cases()[name]
    for word in ((False, True) if name in S.WORD_CASES else (False,)):
        st, got = run(evs, word=word)
        N.check_status(st)
        S.assert_same(got, S.reference(name, evs, word), (name, word))
        assert got["bytes_in"] == 14 * sum(len(e) for e in evs) + 8 * (len(evs) + 1)


def test_random_histories_in_one_call(native):
    evs = S.random_batch()
    st, got = run(evs, word=True)
    N.check_status(st)
    S.assert_same(got, S.reference("random", evs, True), "random")
    assert got["ns_device"] > 0


def test_capacity_exact_and_one_below(native):
    evs = S.cases()["bad_among_good"]
    want = S.reference("bad_among_good", evs, True)
    T = want["n_ops"]
    st, got = run(evs, word=True, ops_cap=T)
    N.check_status(st)
    S.assert_same(got, want, "cap = need")
    ev_off, ev = columns.concat_events(evs)
    guard = {k: np.full(T + 7, 0xA5, dt) for k, dt in (("f", np.uint8), ("a", np.int32), ("b", np.int32), ("process", np.int32), ("inv_pos", np.uint32),
                                                        ("ret_pos", np.uint32), ("word", np.uint32))}
    before = {k: v.copy() for k, v in guard.items()}
    i, o, keep = S.structs(ev_off, ev, T - 1, guard)
    assert native.lib().tbc_pair_events_batch(C.byref(i), C.byref(o)) == N.ERR_INVALID_ARG
    assert f"{T} ops survive" in native.lib().tbc_last_error().decode()
    for k, v in guard.items():
        assert np.array_equal(v, before[k]), k
    # at the exact capacity the words behind the ops stay as they were
    i, o, keep = S.structs(ev_off, ev, T, guard)
    assert native.lib().tbc_pair_events_batch(C.byref(i), C.byref(o)) == 0
    for k, v in guard.items():
        assert np.array_equal(v[:T], want[k]) and np.array_equal(v[T:], before[k][T:]), k


def test_python_surface(native):
    evs = S.cases()["bad_among_good"]
    ops, status, bad_row = columns.pair_events_batch(evs)
    assert [o is None for o in ops] == [True, False, False, True, False, False, True] and list(bad_row[[0, 3, 6]]) == [20, 20, 0]
    for o, e in zip(ops, evs):
        if o is not None:
            h = columns.pair_events(e)
            assert (o.n_events, o.n_process) == (h.n_events, h.n_process)
            for k in ("f", "a", "b", "process", "inv_pos", "ret_pos"):
                assert np.array_equal(getattr(o, k), getattr(h, k)), k


def events_of(seed0, count, n_ops=200, info=0.0, bad_every=5):
    return [synth.register_events(n_ops=n_ops + 17 * (s % 7), n_procs=8, seed=seed0 + s, busy=0.3, info=info, corrupt=0.4 if bad_every and s % bad_every == 0 else 0.0)
            for s in range(count)]


@pytest.mark.parametrize("info, count_form, lanes", [(0.0, False, 8), (0.03, True, 64), (0.03, True, 8)])
def test_reload_events_equals_reload_of_host_paired_columns(native, info, count_form, lanes):
    opts = lambda: core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, want_witness=False, count_form=count_form, lanes_per_history=lanes,
                                  search_width=4 if lanes == 64 and not count_form else 0)
    gm = lambda: core.make_model(N.MODEL_CAS_REGISTER, N.NIL)
    key = lambda r: tuple(r[k] for k in KEYS)
    first = [columns.pair_events(e) for e in events_of(100, 64, info=info)]
    inputs = [events_of(300, 64, info=info, bad_every=4), events_of(500, 57, n_ops=180, info=info)]
    with core.Batch(first, gm(), opts()) as by_events, core.Batch(first, gm(), opts()) as by_ops:
        by_events.run(), by_ops.run()
        for k, evs in enumerate(inputs):
            paired = [columns.pair_events(e) for e in evs]
            by_ops.reload(paired)
            by_events.reload_events(evs)
            want, got = by_ops.run().results(), by_events.run().results()
            assert len(got) == len(evs) and [key(r) for r in got] == [key(r) for r in want], k
            assert {r["valid"] for r in got} >= {0, 1}
            assert by_events.input_info()["total_ops"] == sum(len(h) for h in paired)
            assert by_events.pair_bytes_in == 14 * sum(len(e) for e in evs) + 8 * (len(evs) + 1)
        # a malformed history among them: refused before anything is submitted, the batch still answers its resident input
        spoilt = list(inputs[1])
        spoilt[3] = S.cases()["malformed_each"][2]
        with pytest.raises(N.TbcError) as e:
            by_events.reload_events(spoilt)
        assert e.value.status == N.ERR_BAD_HISTORY and "history 3" in e.value.detail and "row 90" in e.value.detail
        assert by_events.input_info()["pending"] == 0
        assert [key(r) for r in by_events.run().results()] == [key(r) for r in want]

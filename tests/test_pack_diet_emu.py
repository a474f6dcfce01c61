"""The two counting steps of the pack on the CPU, under the emulators of tests/emu, at the shapes where they can go wrong:

* csrc/pack_one_impl.h phase 4 finds the lower lanes of a 64-op chunk that hold an op of the same process by ballots over the bits of
  the slot number (six bits in Batch64Geo, eight in BatchGeo, ten in the one-history forms);
* csrc/open_walk_impl.h phase A2 finds a candidate's place among the keys of its chunk from a bitmap of the keys in LDS, and keeps
  the compare loop for a chunk whose live keys do not fit the bitmap's window.

Every word against the host restatements, as tests/test_pack_one_emu.py and tests/test_walk_emu.py.  Test infrastructure only: the
product has no CPU path."""
import numpy as np
import pytest

import emu
from jepsen_tigerbeetle_amd import _native as N, columns, synth


def _h(n, p, busy, info=0.0, seed=1, **kw):
    return columns.pair_events(synth.register_events(n_ops=n, n_procs=p, seed=seed, busy=busy, info=info, **kw))


# ---- phase 4 of the pack
def _few_processes():
    """2 - 3 processes x 200 ops: some twenty ops of one process in a chunk, a last chunk of 8 ops; and a 1-op history"""
    hs = [_h(200, 2, 1.0, seed=1), _h(200, 3, 0.7, seed=2), _h(200, 3, 1.0, seed=3), _h(1, 1, 0.5, seed=4)]
    assert all(len(np.asarray(h.as_dict()["f"])) % 64 != 0 for h in hs)
    return hs


def _all_slots():
    """64 processes: slots 0, 31, 32 and 63 in use (bit 5 of the slot number, the sign of the low word)"""
    hs = [_h(1000, 64, 0.9, seed=s) for s in (1, 2)]
    for h in hs:
        assert h.n_process == 64 and {0, 31, 32, 63} <= set(np.asarray(h.as_dict()["process"]).tolist())
    return hs


@pytest.mark.parametrize("slots64", [True, False])
def test_same_process_count_few_processes_and_all_slots(slots64):
    hs = _few_processes() + _all_slots()
    for branch in (False, True):
        assert emu.pack_wg_check(hs, branch=branch, slots64=slots64, seed=1 + branch) is None
    assert emu.pack_wg_check(hs, one=True, seed=3) is None
    assert emu.pack_one_check(hs, seed=4) is None


def test_same_process_count_130_processes():
    """slot numbers above 127: the eighth bit in BatchGeo, and the one-history forms' ten"""
    hs = [_h(2000, 130, 0.9, seed=s) for s in (1, 2)]
    for h in hs:
        assert h.n_process == 130 and int(np.asarray(h.as_dict()["process"]).max()) == 129
    assert emu.pack_wg_check(hs, seed=1) is None
    assert emu.pack_wg_check(hs, branch=True, one=True, seed=2) is None
    assert emu.pack_one_check(hs, seed=3) is None


def test_same_process_count_slotless_calls():
    """count form: a crashed call holds no slot and is counted with nobody, the live calls round it keep their places"""
    hs = [_h(200, 3, 1.0, info=0.2, seed=1), _h(300, 16, 0.5, info=0.3, seed=2), _h(130, 4, 1.0, info=0.5, seed=3)]
    assert all((np.asarray(h.as_dict()["ret_pos"]) == 0xFFFFFFFF).sum() > 10 for h in hs)
    assert emu.pack_one_check(hs, count=True, seed=1) is None
    small = [h for h in hs if h.n_process <= 64]
    assert small
    assert emu.pack_wg_check(small, count=True, slots64=True, seed=2) is None
    assert emu.pack_wg_check(hs, count=True, branch=True, seed=3) is None


# ---- phase A2 of the walk
ORDERS = [0, 1, 2, 16, 16 + 24]


def _crowds():
    """chunks of at most 64 candidates (6 processes), of 65 - 128 (40 busy processes) and of more than 128 (58 - 64 slots all busy and the
    71 completions of the window), the last two with crashed calls among the candidates"""
    hs = [_h(300, 6, 0.5, seed=1), _h(400, 40, 1.0, info=0.01, seed=2), _h(400, 58, 1.0, info=0.01, seed=3), _h(400, 64, 0.9, seed=4)]
    assert all(h.n_process <= 64 for h in hs) and hs[2].n_process >= 58
    assert all((np.asarray(h.as_dict()["ret_pos"]) == 0xFFFFFFFF).any() for h in hs[1:3])
    return hs


@pytest.mark.parametrize("order", ORDERS)
def test_places_by_counting_every_word(order):
    hs = _crowds() + _few_processes()
    assert emu.walk_check(hs, 8, branch=True, front="compact", by_ret=order) is None
    assert emu.walk_check(hs, 8, branch=False, front="plain", by_ret=order) is None


def _with_long_calls(h):
    """the history with two more processes whose single :write calls are invoked before everything and complete after everything, the
    lower slot's last: two live keys more than a thousand ranks above the first chunks' lowest, not in table order"""
    d = dict(h.as_dict())
    live = np.asarray(d["ret_pos"], np.uint32) != 0xFFFFFFFF
    last = int(max(np.asarray(d["inv_pos"]).max(), np.asarray(d["ret_pos"])[live].max()))
    n = int(d["n_process"])
    d["inv_pos"] = np.concatenate([[0, 1], np.asarray(d["inv_pos"], np.uint32) + 2]).astype(np.uint32)
    d["ret_pos"] = np.concatenate([[last + 4, last + 3], np.where(live, np.asarray(d["ret_pos"], np.uint32) + 2, 0xFFFFFFFF)]).astype(np.uint32)
    d["f"] = np.concatenate([[N.F_WRITE, N.F_WRITE], np.asarray(d["f"], np.uint8)]).astype(np.uint8)
    d["a"] = np.concatenate([[1, 2], np.asarray(d["a"], np.int32)]).astype(np.int32)
    d["b"] = np.concatenate([[0, 0], np.asarray(d["b"], np.int32)]).astype(np.int32)
    d["process"] = np.concatenate([[n, n + 1], np.asarray(d["process"], np.int32)]).astype(np.int32)
    d["n_process"] = n + 2
    return d


@pytest.mark.parametrize("order", [1, 2, 16, 16 + 24])
def test_places_when_a_key_leaves_the_window(order):
    """two calls open for 1,400 ranks: the first chunks keep the compare loop, the last ones (the keys back inside the window) count"""
    hs = [_with_long_calls(_h(2000, 12, 0.6, seed=1)), _with_long_calls(_h(2000, 40, 1.0, info=0.01, seed=2))]
    assert all(int((np.asarray(d["ret_pos"]) != 0xFFFFFFFF).sum()) > 1300 and d["n_process"] <= 64 for d in hs)
    assert emu.walk_check(hs, 8, branch=True, front="compact", by_ret=order) is None
    assert emu.walk_check(hs, 8, branch=False, front="plain", by_ret=order) is None


def test_a_write_offset_wider_than_the_window():
    """list_order 16 + 600: a :write's key alone is past the bitmap -- every chunk with a live :write keeps the compare loop"""
    assert emu.walk_check(_crowds(), 8, branch=True, front="compact", by_ret=16 + 600) is None

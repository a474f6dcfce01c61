"""The front walk as the kernel launches it -- a wavefront takes a run of consecutive chunks of one history and carries each slot's cursor
from chunk to chunk instead of searching for it (walk::walk_run, csrc/open_walk_impl.h) -- on the CPU under the lane-accurate emulator of
tests/emu, against the host-built tables word for word, with the kernel's own run length and with runs of 2 and 3 chunks.  Beside the
words: no carried cursor differs from the searched one (the emulated build searches as well and counts), and exactly one chunk per
(history, run) searches.  Test infrastructure only: the product has no CPU path."""
import functools

import pytest

from emu import walk_runs
from jepsen_tigerbeetle_amd import synth

import walk_runs_shapes as shapes

K = walk_runs.run_length()
RUNS = sorted({K, 2, 3})


@functools.lru_cache(maxsize=None)
def _small(run):
    return shapes.small_shapes(run)


def _check(hists, vpad, run, **kw):
    bad, n = walk_runs.walk_runs_check(hists, vpad, run=0 if run == K else run, **kw)
    assert bad is None, bad
    assert n["mismatches"] == 0, n
    runs, chunks = walk_runs.expected_counts(hists, run)
    assert (n["runs"], n["chunks"]) == (runs, chunks), (n, runs, chunks)
    assert n["searches"] == runs and n["carried"] == chunks - runs, (n, runs, chunks)


def test_the_kernels_run_length():
    assert K >= 2          # (a run of one chunk would carry nothing)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("front,branch", [("compact", True), ("plain", False), ("wide", False), ("wide", True)])
def test_every_word_with_carried_cursors(run, front, branch):
    """the headline's format (compact + branch lists + twin + look), plain rows, wide records with and without branch lists"""
    _check(_small(run), 8, run, branch=branch, front=front)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("order", [1, 2, 16, 16 + 24])
def test_list_orders(run, order):
    _check(_small(run), 8, run, branch=True, front="compact", by_ret=order)


@pytest.mark.parametrize("run", RUNS)
def test_without_the_optional_tables(run):
    """no lookahead records: a chunk's candidates begin at its first front, not seven ranks before it -- the cursor's other bound"""
    hs = _small(run)
    _check(hs, 8, run, twin=True, look=False, front="plain")
    _check(hs, 8, run, twin=False, look=True, branch=True, front="compact")
    _check(hs, 0, run, twin=False, look=False, front="plain")


@pytest.mark.parametrize("run", RUNS)
def test_wider_rows(run):
    """values up to 9 and up to 30: rows of 16 and 32 entries (the 32-entry instantiation)"""
    for vmax, vpad in ((9, 16), (30, 32)):
        hs = [shapes.gen(300, 24, 0.6, seed=s, n_values=vmax + 1) for s in range(2)] + [shapes.planted()]
        _check(hs, vpad, run, front="plain")
        _check(hs, vpad, run, branch=True, front="wide")


def test_full_size_histories():
    """six of the bench's histories (10k invocations, 64 processes: 157 chunks each) in the headline's format"""
    hs = synth.register_ops_many(range(7000, 7006), n_ops=10000, n_procs=64, busy=0.1, info=0.0)
    _check(hs, 8, K, branch=True, front="compact")

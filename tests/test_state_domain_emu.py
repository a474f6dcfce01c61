"""The kernel bodies the emulator runs, at every value-domain class and from every init of tests/state_domain_shapes.py (one mask word, rule
tables on): K5n (csrc/wgl_narrow_impl.h) at 8, 16 and 32 lanes a history against oracle/wgl_beam.c's schedule for it -- verdict, failing op,
counters, and the witness replayed from the init --, K6w (csrc/jit_sweep_wg_impl.h) record by record against oracle/sweep_ref.c with the first
segment's origin at the init, and the front walk (csrc/open_walk_impl.h) at row lengths 2, 4, 8, 16 and 32 with compact and plain front
records, every word against the host-built tables.  The regression net under the device tests of tests/test_state_domain_gpu.py.
Test infrastructure only: the product has no CPU path."""
import pytest

import state_domain_shapes as S
from emu import walk_lines, walk_sparse
from test_narrow_emu import compare
from oracle import wgl
from test_sweep_wg_emu import _compare as compare_sweep

CAP = 1024          # configs a level set holds in the first pass (csrc/jit_sweep_wg.hip)


@pytest.mark.parametrize("name", S.ONE_WORD_RULES)
def test_the_narrow_body_from_every_init_in_every_class(name):
    case, hists = S.CASES[name], S.histories(name)
    for L in (8, 16, 32):
        got = compare(list(hists), S.om(case), L, kind=case.kind, tag=name, pool_words=4_000_000)
        assert {g["vpad"] for g in got} == {case.cls.vpad} and all(g["rules"] & 3 == 3 for g in got), name
        assert sorted({g["valid"] for g in got}) == ([1] if name == "dom2-init" else [0, 1]), name


@pytest.mark.parametrize("name", S.ONE_WORD_RULES)
def test_the_workgroup_sweep_from_every_init_in_every_class(name):
    """every history cut into windows of 32 completions (the first segment's one origin is the init, every later segment's are the class's
    n_dom states by the open calls), then uncut; rules on; the library's composition of the records ends in the oracle's verdict"""
    case, hists = S.CASES[name], S.histories(name)
    swept = 0
    for i, h in enumerate(hists):
        for seg_target in (32, 0) if i % 4 == 0 else (32,):
            # (crashed calls stay candidates for ever: a level or a sub-round past the sets' 1,024 configs ends its segment "overflow", as the oracle's
            # own sizes say it must; every other record is still compared)
            ref = wgl.check_sweep(h.as_dict(), S.om(case), seg_target=seg_target, n_dom=case.cls.n_dom)
            over = max(ref["max_level"], ref["max_pending"]) > CAP
            assert not over or case.info, (name, i)
            swept += compare_sweep(h, seg_target, case.cls.n_dom, (2, 4, 8)[i % 3], cap=CAP, seed=i, expect_overflow=over, model=S.om(case), vpad=case.cls.vpad)
    assert swept >= len(hists)


@pytest.mark.parametrize("name", [n for n in S.ONE_WORD_RULES if not S.CASES[n].info])
def test_the_front_walk_at_every_row_length(name):
    """the narrow kernel's format (branch lists; the compact record where the class has it, else the wide one) and the wide kernel's (full
    lists, plain rows): the run form the kernel launches and every chunk once more from nothing"""
    case, hists = S.CASES[name], list(S.histories(name))
    vpad = case.cls.vpad
    for kw in (dict(branch=True, front="compact" if case.cls.compact else "wide"), dict(branch=False, front="plain")):
        for order in (0, 16 + 24):
            if vpad <= 8:          # (the stores with lane = entry exist in the <8> walk only)
                bad, n, _, _ = walk_lines.check(hists, vpad=vpad, by_ret=order, **kw)
                assert bad is None and n["mismatches"] == 0 and n["chunks_off"] == 0 and n["no_candidate"] == 0, (name, kw, order, bad, n)
            bad, n = walk_sparse.check(hists, vpad, by_ret=order, **kw)
            assert bad is None and n["mismatches"] == 0, (name, kw, order, bad, n)
            assert (n["sparse"] > 0) is (vpad <= 8), (name, n)          # the <8> walk takes the sparse form, the <32> walk the dense loop
    if case.cls.compact:          # the record the class does NOT get, too: the words are the same tables'
        bad, n, _, _ = walk_lines.check(hists, vpad=vpad, branch=True, front="wide")
        assert bad is None and n["mismatches"] == 0, (name, bad)

"""The cases of tests/state_domain_shapes.py WITHOUT a GPU: every case has the class it is named for (by the restatement of
csrc/batch_create.hip there, by tests/emu's rules_for and by oracle/wgl.py's rules_apply), a by-init case's ops stay below its init and its
histories are ones in which the init matters, the small histories and the hand known-answer histories agree with brute force, every oracle
gives one verdict and one failing op on every history and inside the budgets the device tests pass (nothing undecided, nothing left out), and
every witness replays from the init to the final state the oracle reports.  What tests/test_state_domain_gpu.py compares the kernels with is
pinned here first."""
import numpy as np
import pytest

import emu
import state_domain_shapes as S
from helpers import op_tuples
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.knossos import _analysis
from oracle import brute

MAX_STEPS, MAX_PROBES = 3_000_000, 20_000_000          # tests/test_gpu_parity.py's budgets for the sequential and the wide oracle


def _batch_dict(hists):
    return {k: np.concatenate([np.asarray(getattr(h, k)) for h in hists]) for k in ("f", "a", "b")}


@pytest.mark.parametrize("name", S.NAMES)
def test_every_case_has_the_class_it_is_named_for(native, oracle, name):
    case, hists = S.CASES[name], S.histories(name)
    words = S.mask_words(hists)
    assert words == (2 if case.procs else 1), name
    cls = S.value_class(case.init, hists, words)
    assert cls == case.cls, (name, cls, case.cls)
    assert emu.rules_for(hists, case.kind, case.init) == ((3, cls.vpad) if cls.rules else (0, 0)), name
    assert oracle.rules_apply(_batch_dict(hists), S.om(case)) is cls.rules, name
    vals = np.concatenate([S.values_of(h) for h in hists])
    if case.how == "values":
        assert (int(vals.min()), int(vals.max())) == (case.lo, case.vmax) and case.init == S.NIL, name
        assert set(range(case.lo, case.vmax + 1)) <= set(vals.tolist()) or case.vmax >= 14, name          # (a small domain: every value appears)
    else:
        # the init alone puts the batch where it is: what the ops can write stays below it (two below: the class's last two states are the init's)
        wr = np.concatenate([S.written_values(h) for h in hists] + [np.zeros(0, np.int64)])
        if case.init >= 0:
            assert case.init == case.vmax and (len(wr) == 0 or int(wr.max()) <= max(case.init - 2, 0)) and int(vals.max()) == case.init, name
            assert S.value_class(S.NIL, [h for h in hists if not (S.values_of(h) == case.init).any()], words) != cls or case.vmax > 30, name
        else:
            assert int(vals.min()) == case.init < 0 <= int(wr.min()) and int(vals.max()) == case.vmax, name
    if cls.rules:
        assert cls.n_dom == case.vmax + 2 and cls.vpad >= cls.n_dom > cls.vpad // 2 and cls.walk == (8 if cls.vpad <= 8 else 32), name
        assert cls.compact is (words == 1 and cls.n_dom <= 6) and (cls.n_dom << cls.cut_open) <= S.SWEEP_ORIGINS, name
        assert cls.cut_open == 4 or (cls.n_dom << (cls.cut_open + 1)) > S.SWEEP_ORIGINS, name
        # u64 words of a plain front record: vpad read masks of `words` words, six more, rounded up to a 64 B line
        assert S.front_stride(cls.vpad, words) == {(2, 1): 8, (4, 1): 16, (8, 1): 16, (16, 1): 24, (32, 1): 40, (16, 2): 40, (32, 2): 72}[(cls.vpad, words)], name
    lens = sorted(len(h) for h in hists)
    assert len(hists) >= 8 and (lens[0] <= 8 or case.procs) and lens[-1] >= (120 if case.info else 250), (name, lens)
    if case.info:
        crashed = [S.n_crashed(h) for h in hists]
        assert sum(1 for c in crashed if c >= 2) >= 5, (name, crashed)
        if case.vmax >= 30:          # crashed calls that hold the domain's last values (the valid histories: the last one; the invalid ones: one below)
            top = sum(1 for h in hists if ((np.asarray(h.ret_pos) == S.CRASHED) & (np.asarray(h.a) >= case.vmax - 1)).any())
            assert top >= 6, (name, top)
    else:
        assert all(S.n_crashed(h) == 0 for h in hists), name


def test_the_class_edges_are_all_there():
    """n_dom 2 | 4 | 5, 6 | 7, 8 | 9, 16 | 17, 32 | no tables: both sides of every edge, each by values and by init, and the named extras"""
    doms = {(c.cls.n_dom, c.how) for c in S.CASES.values() if c.cls.rules and not c.procs and not c.info and c.kind == 1}
    assert doms == {(d, how) for d in S.DOMS for how in ("values", "init")}
    assert {S.CASES[n].cls.vpad for n in S.ONE_WORD_RULES} == {2, 4, 8, 16, 32}
    assert {(c.cls.compact, c.cls.walk) for c in S.CASES.values() if c.cls.rules and not c.procs} == {(True, 8), (False, 8), (False, 32)}
    assert {c.cls.cut_open for c in S.CASES.values() if c.cls.rules} == {4, 3, 2}
    for n in ("vmax31-values", "init31", "negative-value", "negative-init", "vmax31-crashed-values", "init31-crashed"):
        assert not S.CASES[n].cls.rules
    assert len(S.TWO_WORDS) == 2 and {S.CASES[n].cls.n_dom for n in S.TWO_WORDS} == {16, 32}
    assert {S.CASES[n].cls.n_dom for n in S.CRASHED_CASES} == {6, 8, 32, 0}


@pytest.mark.parametrize("name", S.BY_INIT)
def test_in_a_by_init_case_the_init_matters(native, oracle, name):
    case, hists = S.CASES[name], S.histories(name)
    here, nil = S.window_refs(name), S.window_refs_under_nil(name)
    differ = [i for i, (r, q) in enumerate(zip(here, nil)) if r["valid"] != q["valid"]]
    assert 3 * len(differ) >= len(hists), (name, differ)
    # the hand shapes: the init taken before any write; a read of it open across the first write; reads of the init and of nil alone, which
    # end in the init with nothing to search; a read of another in-domain value before any write
    R, W, CAS = N.F_READ, N.F_WRITE, N.F_CAS
    h1, h2, h3 = hists[:3]
    assert here[0]["valid"] == here[1]["valid"] == here[2]["valid"] == 1 and nil[0]["valid"] == nil[1]["valid"] == nil[2]["valid"] == 0, name
    assert (h1.f[0], h1.a[0]) == (CAS if case.kind == 1 else R, case.init) and h1.ret_pos[0] < min([h1.inv_pos[i] for i in range(len(h1)) if h1.f[i] == W] + [10 ** 9]), name
    rd = [i for i in range(len(h2)) if h2.f[i] == R and h2.a[i] == case.init][0]
    wr = [i for i in range(len(h2)) if h2.f[i] in (W, CAS)][0]
    assert h2.inv_pos[rd] < h2.inv_pos[wr] and h2.ret_pos[wr] < h2.ret_pos[rd], name
    assert set(h3.f.tolist()) == {R} and set(h3.a.tolist()) == {case.init, S.NIL} and here[2]["final_state"] == case.init, name
    if case.vmax - (2 if case.init >= 0 else 0) >= 0:
        h4 = hists[3]
        assert (h4.f[0], here[3]["valid"], here[3]["fail_op"]) == (R, 0, 0) and h4.a[0] != case.init and h4.a[0] in S.written_values(h4), name
        assert oracle.check(S.histories(name)[3].as_dict(), S.om(case), "window")["valid"] == 0
        fixed = h4.as_dict()
        fixed["a"] = h4.a.copy(); fixed["a"][0] = case.init          # ... its only flaw: with the init read there it is valid
        assert oracle.check(fixed, S.om(case), "window")["valid"] == 1, name


@pytest.mark.parametrize("name", S.NAMES)
def test_the_oracles_agree_and_decide_every_history(native, oracle, name):
    """ref, window, the wide schedule at 1, 4 and 16 configs a round, the narrow one, the sweep cut and uncut, the count form where it applies:
    one verdict, one failing op; every witness replays from the init to the reported final state; nothing is undecided under the budgets"""
    case, hists, model = S.CASES[name], S.histories(name), S.om(S.CASES[name])
    cls = case.cls
    refs = S.window_refs(name)
    verdicts = [r["valid"] for r in refs]
    assert set(verdicts) <= {0, 1}, (name, verdicts)
    if name != "dom2-init":          # (init 0 and nothing to write: the register never leaves its init, no read of 0 or nil can be wrong)
        assert 3 * verdicts.count(0) >= len(hists) and 3 * verdicts.count(1) >= len(hists), (name, verdicts)
    for i, (h, ref) in enumerate(zip(hists, refs)):
        d, tup = h.as_dict(), op_tuples(h)
        want = (ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None)
        if len(h) <= 8:
            bad = brute.first_bad_completion(model, tup)
            assert want == ((1, None) if bad is None else (0, bad)), (name, i)
        runs = {"ref": oracle.check(d, model, "ref", max_steps=MAX_STEPS)}
        for width in (1, 4, 16):
            runs["beam%d" % width] = oracle.check_beam(d, model, width, eager_reads=cls.rules, twin_rule=cls.rules, max_probes=MAX_PROBES)
        for L in (8, 32):
            runs["narrow%d" % L] = oracle.check_beam(d, model, 1, round_pairs=L, rules_at_any_round_size=True, eager_reads=cls.rules, twin_rule=cls.rules,
                                                     branch_lists=cls.rules, max_probes=MAX_PROBES)
        if not case.procs:
            if cls.rules:
                runs["sweep"] = oracle.check_sweep(d, model, seg_target=0, n_dom=cls.n_dom)
                runs["sweep-cut"] = oracle.check_sweep(d, model, seg_target=32, n_dom=cls.n_dom)
                runs["sweep-cut-8"] = oracle.check_sweep(d, model, seg_target=8, n_dom=cls.n_dom)
            else:          # as the library sweeps a batch without tables: one segment, its one origin the init (n_dom 1), no rules
                runs["sweep-no-domain"] = oracle.check_sweep(d, model, eager_reads=False, twin_rule=False, seg_target=0, n_dom=1)
            if ref["valid"] == 1 and not case.info:
                # the state a sweep ends in is one a linearization ends in: knossos.linear as published (linear_ref.c) has them all
                lin = oracle.check_linear(d, model, max_configs=500_000)
                assert lin["valid"] == 1 and lin["n_configs"] <= 4096, (name, i)
                ends = {int(np.int64(s).astype(np.int32)) for s in lin["configs"][:, 0]}
                for how in [k for k in runs if k.startswith("sweep")]:
                    assert runs[how]["final_state"] in ends, (name, i, how, runs[how]["final_state"], ends)
        if case.info:
            cnt = oracle.check_count(d, model, width=4, max_probes=MAX_PROBES)
            if cls.rules:
                assert cnt is not None, (name, i)
                runs["count"] = cnt
                pipe = oracle.check_count_pipeline(d, model, width=4, relaxed_sweep=True)
                assert (pipe[0], pipe[1] if pipe[0] == 0 else None) == want, (name, i, "count pipeline", pipe[4])
            else:          # (the oracle judges one history; the library's gate, the batch: a history that holds no 31 itself has the form here, never there)
                assert (cnt is None) is (not oracle.rules_apply(d, model)), (name, i, "the count form's oracle takes a value or an init it has no class for")
        for how, r in runs.items():
            assert r["valid"] != -1, (name, i, how, "undecided")
            assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == want, (name, i, how, r["valid"], r["fail_op"], want)
            if r["valid"] == 1 and r.get("witness") is not None:
                assert brute.check_witness(model, tup, [int(x) for x in r["witness"]]) == r["final_state"], (name, i, how)
        assert brute.check_witness(model, tup, [int(x) for x in ref["witness"]]) == ref["final_state"] if ref["valid"] == 1 else True, (name, i)


@pytest.mark.parametrize("kat", S.kats(), ids=lambda k: k[0])
def test_hand_histories_against_brute_force(native, oracle, kat):
    name, model, hist, valid, fail_index, msg = kat
    enc = _analysis.Encoded(model, hist)
    m = enc.native_model[0]
    om = {"kind": 1 if m.kind == N.MODEL_CAS_REGISTER else 0, "init": m.init}
    assert m.init == enc.intern.enc(model.value) != S.NIL
    tup = op_tuples(enc.ops)
    bad = brute.first_bad_completion(om, tup)
    assert (bad is None) is valid, name
    if not valid:
        assert int(enc.ops.ret_pos[bad]) == fail_index, name
        # the message a final path ends in is the Python model's own, stepped through a linearization of what completed before
        states = [model]
        for op in (o for o in hist[:fail_index] if o["type"] == "ok"):
            states += [s.step(op) for s in states if not S.M.inconsistent_p(s.step(op))]
        assert msg in {s.step(hist[fail_index]).msg for s in states if S.M.inconsistent_p(s.step(hist[fail_index]))}, name
    for alg in ("ref", "window"):
        r = oracle.check(enc.ops.as_dict(), om, alg)
        assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == ((1, None) if valid else (0, bad)), (name, alg)
    if not valid:
        # the configs stuck at the failing completion (knossos :configs; the surface builds :final-paths from them): each of these histories has
        # exactly one, and both oracles name it.  Where the FIRST completion fails it is the root itself -- the init, nothing linearized --, which
        # the sequential search never puts into its visited set: brute force says why it is stuck (the init does not allow the failing op, and
        # nothing else is open that could go first)
        oracle.check(enc.ops.as_dict(), om, "window")
        seq = oracle.last_configs("window")
        oracle.check_beam(enc.ops.as_dict(), om, 4)
        assert seq == oracle.last_configs("beam") and seq[0] == 1, (name, seq)
        if int((enc.ops.ret_pos < enc.ops.ret_pos[bad]).sum()) == 0:
            assert seq[1] == [[m.init, 0]], (name, seq)
            f, a, b = tup[bad][:3]
            assert brute.step(om, m.init, f, a, b) is None and [i for i, o in enumerate(tup) if o[3] < tup[bad][4]] == [bad], name


def test_the_wire_format_refuses_255_before_it_could_travel_as_nil(native):
    """core.Batch.wire_words: 0xFF is the wire's nil -- a :read of 255 would travel as a read of nil, which every state allows, and the verdict
    come back silently wrong.  Any non-nil `a` outside 0 .. 254 and any `b` of a :cas outside 0 .. 254 is refused; 254 and nil travel."""
    from jepsen_tigerbeetle_amd import core
    R, W, CAS = N.F_READ, N.F_WRITE, N.F_CAS
    col = lambda xs, dt: np.array(xs, dt)
    ok = core.Batch.wire_words(col([R, W, CAS, R, CAS], np.uint8), col([S.NIL, 254, 254, 254, 0], np.int32), col([0, 0, 254, 0, S.NIL], np.int32), col([0, 1, 2, 3, 4095], np.int32))
    assert [(int(w) >> 4) & 0xFF for w in ok] == [0xFF, 254, 254, 254, 0] and [(int(w) >> 12) & 0xFF for w in ok] == [0, 0, 254, 0, 0xFF]
    assert [int(w) & 15 for w in ok] == [R, W, CAS, R, CAS] and int(ok[4]) >> 20 == 4095
    for f, a, b in ((R, 255, 0), (W, 255, 0), (CAS, 255, 1), (CAS, 1, 255), (R, 256, 0), (W, -1, 0), (CAS, 1, -1), (CAS, 1, 300), (R, 2 ** 31 - 1, 0)):
        with pytest.raises(ValueError):
            core.Batch.wire_words(col([R, f], np.uint8), col([S.NIL, a], np.int32), col([0, b], np.int32), col([0, 1], np.int32))
    # (the b column of anything but a :cas does not travel: whatever it holds is no reason to refuse)
    assert (int(core.Batch.wire_words(col([W], np.uint8), col([3], np.int32), col([999], np.int32), col([0], np.int32))[0]) >> 12) & 0xFF == 0
    for p in (-1, 4096):
        with pytest.raises(ValueError):
            core.Batch.wire_words(col([R], np.uint8), col([S.NIL], np.int32), col([0], np.int32), col([p], np.int32))


# ---- multi-register: 4 bits a key, the init the packed map
@pytest.mark.parametrize("case", S.multi_register_cases(), ids=lambda c: c[0])
def test_multi_register_from_a_non_empty_map(native, oracle, case):
    name, init_map, hist = case
    encs = S.encode_multi_register(init_map, hist)
    answers = []
    for how, enc, native_model, om in encs:
        m = native_model[0]
        assert (m.kind, m.init, m.n_keys) == (N.MODEL_MULTI_REGISTER, om["init"], 8), (name, how)
        if how == "direct":          # the packed init is the encoder's own: (code + 1) << 4 * key, keys and codes by first appearance, the map's first
            assert enc.native_model[0].init == om["init"] and [enc.mr_keys[k] for k, _ in sorted(init_map.items())] == [0, 1, 2], name
            assert om["init"] == 0x321
        else:                        # key 7 at the 14th value: bits 28 .. 31 = 0xE -- bit 31 and bit 30 (kHotBit in the count form's state word) both set
            assert (om["init"] & 0xFFFFFFFF) >> 28 == 0xE and om["init"] < 0, (name, hex(om["init"]))
            assert enc.mr_keys["k7"] == 7 and enc.intern.enc(S.MR_INIT["k7"]) == 13, name
            pool = enc.ops.pool.reshape(-1, 3)
            assert int(pool[:, 2].max()) == 13 and set(pool[:, 1].tolist()) == set(range(8)), name          # 14 distinct values, 8 keys
            assert ((pool[:, 1] == 7) & (pool[:, 2] >= 7)).any(), name                                       # values 7 .. 13 on key 7
        d, tup = enc.ops.as_dict(), op_tuples(enc.ops)
        ref = oracle.check(d, om, "window", max_steps=5_000_000)
        assert ref["valid"] in (0, 1), (name, how)
        for width in (4, 16):
            r = oracle.check_beam(d, om, width, max_probes=MAX_PROBES)
            assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == (ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None), (name, how, width)
            if r["valid"] == 1:
                assert brute.check_witness(om, tup, [int(x) for x in r["witness"]]) & 0xFFFFFFFF == r["final_state"] & 0xFFFFFFFF, (name, how, width)
        if ref["valid"] == 1:
            assert brute.check_witness(om, tup, [int(x) for x in ref["witness"]]) & 0xFFFFFFFF == ref["final_state"] & 0xFFFFFFFF, (name, how)
        answers.append((ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None, len(enc.ops)))
        # the history reads the whole initial map before any write is invoked: under the empty map that read is the failing op
        empty = oracle.check(d, dict(om, init=0), "window", max_steps=5_000_000)
        assert (empty["valid"], empty["fail_op"]) == (0, 0), (name, how)
    assert answers[0] == answers[1], name                    # one map, two numberings: one answer
    assert answers[0][0] == (0 if "stale" in name else 1), name


def test_multi_register_past_the_direct_model_goes_to_the_memo_table(native, oracle):
    """15 distinct values; 9 keys: knossos/_analysis.py falls back to the memo table, and the table's verdict is brute force's over the same
    table -- and, for the histories as generated (no stale read planted), valid"""
    n_bad = 0
    for name, init_map, hist in S.multi_register_fallbacks():
        enc = _analysis.Encoded(S.M.multi_register(dict(init_map)), hist)
        assert enc.native_model[0].kind == N.MODEL_TABLE, name
        om = {"kind": 3, "init": 0, "table": enc.table_info["table"]}
        tup = op_tuples(enc.ops)
        assert len(tup) <= 9, name
        bad = brute.first_bad_completion(om, tup)
        n_bad += bad is not None
        assert (bad is None) or name[-1] in "13", name          # (only a planted stale read makes one invalid)
        for alg in ("ref", "window"):
            r = oracle.check(enc.ops.as_dict(), om, alg)
            assert (r["valid"], r["fail_op"] if r["valid"] == 0 else None) == ((1, None) if bad is None else (0, bad)), (name, alg)
    assert n_bad >= 2
    # one value fewer / one key fewer: the direct model
    name, init_map, hist = S.multi_register_cases()[0]
    assert _analysis.Encoded(S.M.multi_register(dict(init_map)), hist).native_model[0].kind == N.MODEL_MULTI_REGISTER

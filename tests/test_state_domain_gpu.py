"""Initial values and value-domain classes ON THE DEVICE, every engine against the oracle of its schedule through the C-ABI (the cases, their
classes and the sequential references are tests/state_domain_shapes.py's; tests/test_state_domain_oracle.py pins them and the oracles without
a GPU, tests/test_state_domain_emu.py runs the emulated kernel bodies over them).

The model's init is read by the root of every search (wgl_search.hip, wgl_beam.hip, wgl_narrow_impl.h), by the first segment's origin of the
sweep (jit_sweep.hip, jit_sweep_wg_impl.h), by the witness replay (witness_expand.h), by final_state of a history with nothing to search and
by the count form's gate -- and, as the batch's largest value, it picks n_dom / vpad and with them the front record, the walk kernel, the
records' stride and the sweep's cut_open.  Every comparison is equality: verdict, failing op, the op before it, witness (replayed from the init
by oracle/brute.py), final state and every counter; no history of any case is left out."""
import numpy as np
import pytest

import state_domain_shapes as S
from batch_size_shapes import renamed, sequential
from helpers import _assert_narrow, assert_same, op_tuples
from jepsen_tigerbeetle_amd import _native as N, core
from jepsen_tigerbeetle_amd.jepsen import checker as jc
from oracle import brute

pytestmark = pytest.mark.gpu

MAX_PROBES = 20_000_000
KEYS = ("valid", "fail_op", "prev_ok_op", "probes", "visited", "backtracks", "max_depth", "steps", "final_state")      # (tests/test_stream_gpu.py's)
ONE_WORD = tuple(n for n in S.NAMES if not S.CASES[n].procs)


def opts(**kw):
    return core.make_opts(time_limit_ms=60000, **kw)


def key(r):
    return tuple(r[k] for k in KEYS)


def replay(case, h, got, tag):
    assert brute.check_witness(S.om(case), op_tuples(h), [int(x) for x in got["witness"]]) == got["final_state"], tag


def beam_expect(oracle, case, h, width, **kw):
    """the wide schedule under the rules the BATCH has (the oracle alone would judge by the one history's values)"""
    e = oracle.check_beam(h.as_dict(), S.om(case), width, eager_reads=case.cls.rules, twin_rule=case.cls.rules, max_probes=MAX_PROBES, **kw)
    assert e["valid"] != -1
    return e


def narrow_expect(oracle, case, h, L, rules=None, **kw):
    rules = case.cls.rules if rules is None else rules
    e = oracle.check_beam(h.as_dict(), S.om(case), 1, round_pairs=L, rules_at_any_round_size=True, eager_reads=rules, twin_rule=rules, branch_lists=rules,
                          max_probes=MAX_PROBES, **kw)
    assert e["valid"] != -1
    return e


def assert_wide(case, h, got, exp, tag):
    assert got["valid"] == exp["valid"], (tag, got["valid"], exp["valid"], got["cause"])
    if exp["valid"] == 0:
        assert got["fail_op"] == exp["fail_op"], tag
        assert got["prev_ok_op"] == (None if exp["prev_ok_op"] == N.NO_OP else exp["prev_ok_op"]), tag
    else:
        assert got["final_state"] == exp["final_state"], tag
        assert np.array_equal(got["witness"], exp["witness"]), tag
        replay(case, h, got, tag)
    assert (got["probes"], got["visited"], got["backtracks"], got["max_depth"]) == (exp["probes"], exp["visited"], exp["expanded"], exp["max_stack"]), tag


# ---- K3: the sequential kernel (wgl_search.hip)
@pytest.mark.parametrize("name", S.NAMES)
def test_sequential_kernel(native, oracle, name):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    with core.Batch(list(hists), S.gm(case), opts(algorithm=N.ALG_WGL)) as b:
        res = b.run().results()
    for i, (h, got, exp) in enumerate(zip(hists, res, refs)):
        assert got["search_width"] == 1, (name, i)
        assert_same(got, exp, (name, i))
        if exp["valid"] == 1:
            replay(case, h, got, (name, i))


# ---- K5: the wide kernel (wgl_beam.hip)
@pytest.mark.parametrize("width", [2, 4, 16])
@pytest.mark.parametrize("name", S.NAMES)
def test_wide_kernel(native, oracle, name, width):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    with core.Batch(list(hists), S.gm(case), opts(algorithm=N.ALG_COMPETITION, search_width=width)) as b:
        assert (b.search_width(), b.lanes_per_history()) == (width, 64), name
        res = b.run().results()
    for i, (h, got, ref) in enumerate(zip(hists, res, refs)):
        exp = beam_expect(oracle, case, h, width)
        assert (exp["valid"], exp["fail_op"] if exp["valid"] == 0 else None) == (ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None), (name, i)
        assert_wide(case, h, got, exp, (name, width, i))


# ---- K5n: several histories per wavefront (wgl_narrow.hip), the witness expanded on the host from the init (witness_expand.h)
@pytest.mark.parametrize("L", [8, 16, 32])
@pytest.mark.parametrize("name", S.NAMES)
def test_narrow_kernel(native, oracle, name, L):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    with core.Batch(list(hists), S.gm(case), opts(algorithm=N.ALG_COMPETITION, lanes_per_history=L)) as b:
        assert (b.lanes_per_history(), b.search_width()) == (L, 1), name
        res = b.run().results()
    for i, (h, got, ref) in enumerate(zip(hists, res, refs)):
        exp = narrow_expect(oracle, case, h, L)
        assert exp["valid"] == ref["valid"], (name, i)
        _assert_narrow(got, exp, (name, L, i))
        if exp["valid"] == 1:
            assert got["witness"] is not None and np.array_equal(got["witness"], exp["witness"]), (name, L, i)
            replay(case, h, got, (name, L, i))


# ---- the level sweep (jit_sweep.hip, jit_sweep_wg.hip): the first segment's origin is the init, the cuts enumerate the class's n_dom states
@pytest.mark.parametrize("rules", [True, False], ids=["rules", "no-rules"])
@pytest.mark.parametrize("name", ONE_WORD)
def test_level_sweep(native, oracle, name, rules):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    cls = case.cls
    with core.Batch(list(hists), S.gm(case), opts(algorithm=N.ALG_LINEAR, want_witness=False, eager_reads=rules, twin_rule=rules)) as b:
        res = b.run().results()
        info = b.sweep_info()
        again = b.run().results()
    assert info["enabled"] == 1, name
    if cls.rules:
        assert (info["n_dom"], info["cut_open"]) == (cls.n_dom, cls.cut_open) and info["seg_target"] >= 32, (name, info)
    else:          # no value domain to enumerate a cut's configs from: ONE segment a history, its one origin the init (n_dom 1), swept without the rules
        assert (info["n_dom"], info["seg_target"], info["max_segs"], info["cut_open"]) == (1, 0, 1, 0), (name, info)
    n_swept = 0
    for i, (h, got, ref) in enumerate(zip(hists, res, refs)):
        assert got["valid"] == ref["valid"], (name, i, got["cause"])
        if ref["valid"] == 0:
            assert got["fail_op"] == ref["fail_op"], (name, i)
        assert key(again[i]) == key(got), (name, i)
        if got["analyzer"] != N.ALG_LINEAR:          # handed to the depth-first search (a level outgrew the sets): the verdict and the failing op above are all there is to compare
            continue
        n_swept += 1
        on = rules and cls.rules
        exp = oracle.check_sweep(h.as_dict(), S.om(case), eager_reads=on, twin_rule=on, seg_target=info["seg_target"], n_dom=info["n_dom"])
        assert got["valid"] == exp["valid"], (name, i)
        if exp["valid"] == 0:
            assert got["fail_op"] == exp["fail_op"], (name, i)
            assert got["prev_ok_op"] == (None if exp["prev_ok_op"] == N.NO_OP else exp["prev_ok_op"]), (name, i)
            assert got["configs"], (name, i)
        else:
            assert got["final_state"] == exp["final_state"], (name, i, got["final_state"], exp["final_state"])
        assert (got["visited"], got["probes"], got["backtracks"], got["max_depth"]) == (exp["configs_total"], exp["probes"], exp["subrounds"], exp["max_level"]), (name, i)
    assert n_swept >= (len(hists) - 3 if rules and not case.info else 4), (name, n_swept)


# ---- the count form (crashed calls as counts per effect class): on where the class has tables, off -- the mask form answers -- at 31
@pytest.mark.parametrize("name", S.CRASHED_CASES)
def test_count_form_or_the_mask_form_where_it_is_off(native, oracle, name):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    budget = 32 * max(len(h) for h in hists)
    with core.Batch(list(hists), S.gm(case), opts(algorithm=N.ALG_COMPETITION, search_width=4, count_form=True)) as b:
        res = b.run().results()
    for i, (h, got, ref) in enumerate(zip(hists, res, refs)):
        if case.cls.rules:
            v, fo, last, tot, how = oracle.check_count_pipeline(h.as_dict(), S.om(case), width=4, budget=budget, want_witness=True)
            assert (v, fo if v == 0 else None) == (ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None), (name, i, how)
            assert got["valid"] == v, (name, i, how)
            assert (got["probes"], got["visited"], got["backtracks"]) == (tot["probes"], tot["visited"], tot["expanded"]), (name, i, how)
            if v == 1:
                assert np.array_equal(got["witness"], last["witness"]) and got["final_state"] == last["final_state"], (name, i)
                replay(case, h, got, (name, i))
            else:
                assert got["fail_op"] == fo, (name, i, how)
        else:          # a value or an init of 31: no classes -- asked for or not, the search is the mask form's, counter by counter
            assert_wide(case, h, got, beam_expect(oracle, case, h, 4), (name, "mask form", i))
    # a handful of histories, nobody asking for a witness or a schedule: the relaxed level sweep and its reach table run first
    few = list(hists[4:12])
    with core.Batch(few, S.gm(case), opts(algorithm=N.ALG_COMPETITION, want_witness=False, count_form=True)) as b:
        res = b.run().results()
    for i, (h, got, ref) in enumerate(zip(few, res, refs[4:12])):
        assert (got["valid"], got["fail_op"]) == (ref["valid"], ref["fail_op"] if ref["valid"] == 0 else None), (name, "few", i)
        if case.cls.rules:
            exp = oracle.check_count_pipeline(h.as_dict(), S.om(case), width=got["search_width"], budget=32 * max(len(x) for x in few), relaxed_sweep=True)
            assert (got["valid"], got["probes"], got["visited"]) == (exp[0], exp[3]["probes"], exp[3]["visited"]), (name, "few", i, exp[4])


# ---- tbc_check, one history: pack_one's sixteen wavefronts, its own rk8 and front records; the class is the history's own (and the init's)
@pytest.mark.parametrize("name", S.NAMES)
def test_one_history_through_tbc_check(native, oracle, name):
    case, hists, refs = S.CASES[name], S.histories(name), S.window_refs(name)
    for i in ((1, 2, 6) if case.how == "init" else (0, 4, 6)):
        h = hists[i]
        own = S.value_class(case.init, [h], S.mask_words([h]))
        got = core.check_ops(h, S.gm(case), opts(algorithm=N.ALG_WGL))
        assert_same(got, refs[i], (name, i))
        got = core.check_ops(h, S.gm(case), opts(algorithm=N.ALG_COMPETITION, search_width=4))
        exp = oracle.check_beam(h.as_dict(), S.om(case), 4, eager_reads=own.rules, twin_rule=own.rules, max_probes=MAX_PROBES)
        assert_wide(case, h, got, exp, (name, "wide", i))
        got = core.check_ops(h, S.gm(case), opts(algorithm=N.ALG_COMPETITION, lanes_per_history=8))
        _assert_narrow(got, narrow_expect(oracle, case, h, 8, rules=own.rules), (name, "narrow", i))
        if own.rules and S.mask_words([h]) == 1:
            got = core.check_ops(h, S.gm(case), opts(algorithm=N.ALG_LINEAR, want_witness=False))
            assert (got["valid"], got["fail_op"]) == (refs[i]["valid"], refs[i]["fail_op"] if refs[i]["valid"] == 0 else None), (name, "sweep", i)
            if refs[i]["valid"] == 1 and got["analyzer"] == N.ALG_LINEAR:
                assert got["final_state"] == oracle.check_sweep(h.as_dict(), S.om(case), seg_target=0, n_dom=own.n_dom)["final_state"], (name, "sweep", i)


# ---- fresh inputs (batch_stream.hip): the value domain of a batch is its first input's AND its init's
NARROW = dict(algorithm=N.ALG_COMPETITION, want_witness=False, lanes_per_history=8)


def fresh(hists, case, o):
    with core.Batch(list(hists), S.gm(case), o) as b:
        return [key(r) for r in b.run().results()]


def fitting(nxt, first):
    """the longest prefix of nxt that a batch created from `first` has room for"""
    room, out = sum(len(h) for h in first), []
    for h in nxt:
        if sum(len(x) for x in out) + len(h) <= room and len(out) < len(first):
            out.append(h)
    return out


@pytest.mark.parametrize("d", S.DOMS)
@pytest.mark.parametrize("created", ["init", "values"])
def test_a_batch_takes_a_fresh_input_of_its_class_built_the_other_way(native, oracle, d, created):
    """created by init (ops 0 .. vmax - 2, init = vmax) it takes the by-values input that holds vmax = n_dom - 2 itself, and the other way
    round; n_dom - 1 is refused by name even where vpad has a row for it (n_dom 5, 7, 9, 17), and afterwards the batch is as good as new"""
    other = "values" if created == "init" else "init"
    case, first = S.CASES[f"dom{d}-{created}"], list(S.histories(f"dom{d}-{created}"))
    nxt = fitting(S.histories(f"dom{d}-{other}"), first)
    assert len(nxt) >= 8 and int(max(S.values_of(h).max() for h in nxt if len(S.values_of(h)))) == d - 2
    o = opts(**NARROW)
    with core.Batch(first, S.gm(case), o) as b:
        res = b.run().results()
        before = [key(r) for r in res]
        for i, h in enumerate(first):
            _assert_narrow(res[i], narrow_expect(oracle, case, h, 8, want_witness=False), (d, "created", i))
        b.reload(nxt)
        res = b.run().results()
        assert [key(r) for r in res] == fresh(nxt, case, o)          # (under the BATCH's model: the other case's histories from this case's init)
        for i, h in enumerate(nxt):
            _assert_narrow(res[i], narrow_expect(oracle, case, h, 8, want_witness=False), (d, "reloaded", i))
        assert b.input_info()["inputs_consumed"] == 1
        for bad in (nxt[:-1] + [sequential([(N.F_CAS, 0, d - 1)])], [sequential([(N.F_WRITE, d - 1, 0)])] + nxt[:-1]):
            b.reload(bad)
            with pytest.raises(N.TbcError) as err:
                b.run()
            assert err.value.status == N.ERR_UNSUPPORTED and "value domain" in err.value.detail, d
        b.reload(first)
        assert [key(r) for r in b.run().results()] == before


def test_a_batch_without_tables_takes_a_wire_value_of_254(native, oracle):
    """values past 30: no rows to index, so everything the wire format holds travels -- through tbc_batch_reload and through a mapped slot
    filled by core.Batch.wire_words (which refuses 255, the wire's nil: tests/test_state_domain_oracle.py)"""
    case = S.CASES["vmax31-values"]
    first = list(S.histories("vmax31-values"))
    nxt = [renamed(h) for h in first[:-1]] + [sequential([(N.F_READ, N.NIL, 0), (N.F_WRITE, 254, 0), (N.F_CAS, 254, 254), (N.F_READ, 254, 0)])]
    assert max(int(S.values_of(h).max()) for h in nxt) == 254
    o = opts(**NARROW)
    want = fresh(nxt, case, o)
    refs = [oracle.check(h.as_dict(), S.om(case), "window", want_witness=False) for h in nxt]
    assert [(w[0], w[1]) for w in want] == [(r["valid"], r["fail_op"] if r["valid"] == 0 else None) for r in refs]
    assert want[-1][0] == 1 and want[-1][-1] == 254
    with core.Batch(first, S.gm(case), o) as b:
        b.run(want_results=False)
        b.reload(nxt)
        assert [key(r) for r in b.run().results()] == want
        b.submit_input(1, b.fill_input(1, nxt))
        assert [key(r) for r in b.run().results()] == want
        assert b.input_info()["inputs_consumed"] == 2


# ---- the knossos / jepsen surface
@pytest.mark.parametrize("kat", S.kats(), ids=lambda k: k[0])
def test_hand_histories_through_the_checker_surface(native, kat):
    name, model, hist, valid, fail_index, msg = kat
    for alg in ("wgl", "linear", None):
        a = jc.linearizable({"model": model, "algorithm": alg}).check(None, hist, None)
        assert a["valid?"] is valid, (name, alg)
        if valid:
            assert a["configs"] and isinstance(a["configs"][0]["model"], type(model)), (name, alg)
            continue
        assert a["op"]["index"] == fail_index and a["op"]["type"] == "ok", (name, alg)
        assert a["final-paths"], (name, alg)
        last = a["final-paths"][0][-1]
        assert last["op"]["index"] == fail_index and last["model"].msg == msg, (name, alg, last["model"].msg)
    if not valid:          # the state the stuck config holds is decoded through the same interning as the init: the model the message names
        assert any(str(c["model"].value) == msg.rsplit(" ", 1)[1] for c in a["configs"]), (name, a["configs"])


# ---- multi-register: the packed initial map, key 7 at the 14th value (bits 28 .. 31 of the state word)
@pytest.mark.parametrize("case", S.multi_register_cases(), ids=lambda c: c[0])
def test_multi_register_from_a_non_empty_map(native, oracle, case):
    name, init_map, hist = case
    for how, enc, native_model, om in S.encode_multi_register(init_map, hist):
        d, tup = enc.ops.as_dict(), op_tuples(enc.ops)
        exp = oracle.check(d, om, "window", max_steps=5_000_000)
        assert exp["valid"] != -1
        got = core.check_ops(enc.ops, native_model, opts())
        assert_same(got, exp, (name, how))
        for width in (4, 16):
            for eager, indep in ((True, True), (True, False), (False, True)) if width == 4 else ((True, True),):
                expb = oracle.check_beam(d, om, width, eager_txns=eager, txn_independence=indep, max_probes=MAX_PROBES)
                gotb = core.check_ops(enc.ops, native_model, opts(algorithm=N.ALG_COMPETITION, search_width=width, eager_txns=eager, txn_independence=indep))
                tag = (name, how, width, eager, indep)
                assert gotb["valid"] == expb["valid"] == exp["valid"], tag
                assert (gotb["probes"], gotb["visited"], gotb["backtracks"], gotb["max_depth"]) == (expb["probes"], expb["visited"], expb["backtracks"], expb["max_depth"]), tag
                if exp["valid"] == 1:
                    assert np.array_equal(gotb["witness"], expb["witness"]) and gotb["final_state"] == expb["final_state"], tag
                    assert brute.check_witness(om, tup, [int(x) for x in gotb["witness"]]) & 0xFFFFFFFF == gotb["final_state"] & 0xFFFFFFFF, tag
                else:
                    assert gotb["fail_op"] == exp["fail_op"], tag

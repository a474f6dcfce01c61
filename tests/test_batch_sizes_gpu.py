"""Every pack, sizing and list-placing path at each batch-size class, on the MI355X against the oracles (tests/batch_size_shapes.py has
the families, the sizes and the references; tests/test_batch_sizes_oracle.py checks them without a GPU).

The number of histories decides which kernels pack a batch, with how many threads, who sizes the per-front lists, how
stream_assign_lists_kernel deals their places and how often the grid loops of pack_kernel / open_counts_kernel / open_dprod_kernel /
count_fronts_kernel go round.  A history's answer must depend on none of it: EVERY history of every batch is compared with the oracle's
statement of its schedule -- verdict, failing op, every counter -- so that a wrong stride, a table not cleared between two trips of a
grid loop or a list placed one entry off shows as a counter that differs (nothing is planted on the device)."""
import pytest

import batch_size_shapes as S
from jepsen_tigerbeetle_amd import _native as N, core

pytestmark = pytest.mark.gpu

KEYS = ("valid", "fail_op", "prev_ok_op", "probes", "visited", "backtracks", "max_depth", "steps", "final_state", "search_width")


def gm():
    return core.make_model(N.MODEL_CAS_REGISTER, N.NIL)


def keys(res):
    return [tuple(r[k] for k in KEYS) for r in res]


def assert_as_the_oracle(name, res, exp, tag, fell_back=()):
    """every history's result against its reference, as the family's parity test compares them (helpers._assert_narrow,
    test_gpu_parity.test_wide_schedule_matches_its_oracle, test_count_form_gpu): the verdict, the failing op, the final state, and
    probes / visited / backtracks (= configs expanded) / max_depth (= the deepest stack; not summed over the count form's passes).
    fell_back: histories the sequential kernel answered -- the verdict and the failing op are the history's; the counters and the
    linearization it ends in (the final state) are that search's own."""
    kind = S.FAMILIES[name].kind
    narrow = "lanes_per_history" in S.FAMILIES[name].opts
    assert len(res) == len(exp), tag
    for i, (g, e) in enumerate(zip(res, exp)):
        assert g["valid"] != N.UNKNOWN, (tag, i, g["cause"])
        assert g["valid"] == e["valid"], (tag, i, g["valid"], e["valid"])
        if e["valid"] == 0:
            assert g["fail_op"] == e["fail_op"], (tag, i)
        if i in fell_back:
            continue
        if e["valid"] == 1:
            assert g["final_state"] == e["final_state"], (tag, i)
        if kind == "count":
            assert (g["probes"], g["visited"], g["backtracks"]) == (e["probes"], e["visited"], e["backtracks"]), (tag, i)
        else:
            assert g["search_width"] == (1 if narrow else 4), (tag, i)
            assert (g["probes"], g["visited"], g["backtracks"], g["max_depth"]) == (e["probes"], e["visited"], e["backtracks"], e["max_depth"]), (tag, i)


def assert_schedule(name, b):
    narrow = "lanes_per_history" in S.FAMILIES[name].opts
    assert (b.lanes_per_history(), b.search_width()) == ((8, 1) if narrow else (64, 4)), name


def _created_cases():
    cases = []
    for name in S.SIZE_FAMILIES:
        sizes = S.LONG_SIZES if S.FAMILIES[name].long_neighbour else S.SIZES if name in S.ALL_SIZES_FAMILIES else S.FEW_SIZES
        cases += [(n, name) for n in sizes]
    order = list(S.SIZE_FAMILIES)
    return sorted(cases, key=lambda c: (c[0], order.index(c[1])))          # by size ascending: the first failure is at the smallest batch that shows it


# ---- (a) created batches
@pytest.mark.parametrize("n,name", _created_cases(), ids=lambda v: str(v))
def test_a_created_batch_of_every_size_class_answers_as_the_oracle(native, oracle, n, name):
    hists = S.batch_of(name, n)
    exp = S.expected(oracle, name, hists, S.indices(n))
    with core.Batch(hists, gm(), S.make_opts(name)) as b:
        assert_schedule(name, b)
        res = b.run().results()
        again = b.run().results()
    assert_as_the_oracle(name, res, exp, (name, n))
    assert keys(again) == keys(res)


# ---- (b) fresh inputs across the classes
@pytest.mark.parametrize("name,n_create,n_reload,t_mod4", S.reload_cases(), ids=lambda v: str(v))
def test_a_fresh_input_of_another_size_class_answers_as_the_oracle(native, oracle, name, n_create, n_reload, t_mod4):
    first, idx0, (nxt, idx, which) = S.reload_plan(name, n_create, n_reload, t_mod4)
    total = sum(len(h) for h in nxt)
    assert total % 4 == t_mod4                             # (over the cases: 0, 1, 2 and 3 -- tests/test_batch_sizes_oracle.py)
    with core.Batch(first, gm(), S.make_opts(name)) as b:
        assert_schedule(name, b)
        assert_as_the_oracle(name, b.run().results(), S.expected(oracle, name, first, idx0), (name, "created", n_create))
        b.reload(nxt)
        res = b.run().results()
        assert_as_the_oracle(name, res, S.expected(oracle, name, nxt, idx, which), (name, "reloaded", n_create, n_reload))
        info = b.input_info()
        assert (info["n_hist"], info["pending"], info["inputs_consumed"], info["bytes_copied"]) == (n_reload, 0, 1, 12 * total)
        assert keys(b.run().results()) == keys(res)          # the resident input once more: its lists' places are dealt again on the device
        assert b.input_info()["inputs_consumed"] == 1


@pytest.mark.parametrize("name", ["narrow-1w", "count-wide"])
def test_two_inputs_wait_of_1025_and_of_9_histories(native, oracle, name):
    first = S.batch_of(name, 1025)
    big, idx_big, which_big = S.reload_arrangement(name, 1025, rot=5, t_mod4=2)
    few, idx_few, which_few = S.reload_arrangement(name, 9, rot=23, t_mod4=1)
    with core.Batch(first, gm(), S.make_opts(name)) as b:
        b.run(want_results=False)
        b.submit_input(1, b.fill_input(1, big))
        b.submit_input(2, b.fill_input(2, few))
        assert b.input_info()["pending"] == 2
        assert_as_the_oracle(name, b.run().results(), S.expected(oracle, name, big, idx_big, which_big), (name, "first waiting"))
        info = b.input_info()
        assert (info["n_hist"], info["pending"], info["inputs_consumed"], info["bytes_copied"]) == (1025, 1, 1, 12 * sum(len(h) for h in big))
        res = b.run().results()
        assert_as_the_oracle(name, res, S.expected(oracle, name, few, idx_few, which_few), (name, "second waiting"))
        info = b.input_info()
        assert (info["n_hist"], info["pending"], info["inputs_consumed"], info["bytes_copied"]) == (9, 0, 2, 12 * sum(len(h) for h in few))
        assert keys(b.run().results()) == keys(res)


# ---- (c) lists that outgrow the arena behind 1,024 histories
def test_lists_outgrow_the_arena_in_the_middle_of_a_threads_run_of_histories(native, oracle):
    """stream_assign_lists_kernel at two histories a thread: the running sum of the lists' lengths passes the arena's end at an odd
    history, the second of its thread's run.  That history and every one behind it -- a contiguous suffix, since the sum only grows --
    are answered by the sequential kernel this once (search_width != 1); the place is the one the lengths predict; the arena grows
    once, and the same input again is the narrow kernel's from end to end."""
    name = "dense-narrow"
    quiet, dense, idx = S.overflow_batches()
    n = S.OVERFLOW_N
    per = (n + 1023) // 1024
    exp = S.expected(oracle, name, dense, idx)
    with core.Batch(quiet, gm(), S.make_opts("quiet-narrow")) as b:
        assert_schedule(name, b)
        assert_as_the_oracle("quiet-narrow", b.run().results(), S.expected(oracle, "quiet-narrow", quiet, S.indices(n)), "quiet")
        b.reload(dense)
        res = b.run().results()
        fell = [i for i, r in enumerate(res) if r["search_width"] != 1]
        assert fell and len(fell) < n and fell == list(range(fell[0], n)), (len(fell), fell[:4], fell[-4:])
        assert fell[0] % per != 0 and fell[0] == S.fallback_start(quiet, dense), fell[0]
        assert_as_the_oracle(name, res, exp, "dense, first time", fell_back=set(fell))
        seq = {}
        for i in fell:          # ... which for a valid history is the sequential oracle's
            if res[i]["valid"] == 1:
                if idx[i] not in seq:
                    seq[idx[i]] = oracle.check(dense[i].as_dict(), S.CAS, "window", want_witness=False)
                assert (seq[idx[i]]["valid"], seq[idx[i]]["final_state"]) == (1, res[i]["final_state"]), i
        assert b.input_info()["lists_regrown"] == 1
        b.reload(dense)
        res = b.run().results()
        assert_as_the_oracle(name, res, exp, "dense, again")
        assert b.input_info()["lists_regrown"] == 1 and b.input_info()["inputs_consumed"] == 2


# ---- (d) the wire format's edges through stream_unpack_kernel
def test_value_254_and_nil_travel_in_the_vector_path_and_in_the_scalar_tail(native, oracle):
    name = "values-past-30-wide"
    first = S.batch_of(name, 65)
    nxt = S.wire_edge_input(65)
    refs, exp = {}, []
    for h in nxt:
        if id(h) not in refs:
            refs[id(h)] = S.reference(oracle, name, h)
        exp.append(refs[id(h)])
    assert exp[-1]["valid"] == 1 and exp[-1]["final_state"] == 254 and {e["valid"] for e in exp} == {0, 1}
    with core.Batch(first, gm(), S.make_opts(name)) as b:
        b.run(want_results=False)
        b.reload(nxt)
        res = b.run().results()
        assert_as_the_oracle(name, res, exp, "254")
        assert b.input_info()["bytes_copied"] == 12 * sum(len(h) for h in nxt)


def test_one_value_beyond_the_tables_is_refused_in_the_last_op_and_in_the_first(native, oracle):
    """a batch WITH rule tables (values to 12: rows nil, 0 .. 12): 13 as `b` of a :cas that is the input's very last op and alone in the
    scalar tail, then 13 as `a` of the input's first op -- each the input's only value out of the domain"""
    name = "narrow-1w"
    first, idx0 = S.batch_of(name, 65), S.indices(65)
    good, idx, which = S.reload_arrangement(name, 64, rot=17, t_mod4=0)
    assert S.largest_value(first) == S.largest_value(good) == 12
    last_op_bad = good + [S.sequential([(N.F_CAS, 1, 13)])]
    first_op_bad = [S.sequential([(N.F_WRITE, 13, 0)])] + good
    assert sum(len(h) for h in last_op_bad) % 4 == 1
    with core.Batch(first, gm(), S.make_opts(name)) as b:
        before = b.run().results()
        assert_as_the_oracle(name, before, S.expected(oracle, name, first, idx0), "created")
        for bad in (last_op_bad, first_op_bad):
            b.reload(bad)
            with pytest.raises(N.TbcError) as e:
                b.run()
            assert e.value.status == N.ERR_UNSUPPORTED and "value domain" in e.value.detail
        b.reload(good)
        assert_as_the_oracle(name, b.run().results(), S.expected(oracle, name, good, idx, which), "good input after the refused ones")
        b.reload(first)
        assert keys(b.run().results()) == keys(before)

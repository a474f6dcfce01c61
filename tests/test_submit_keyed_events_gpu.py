"""tbc_batch_map_keyed_events / tbc_batch_submit_keyed_events on the MI355X (core.Batch.map_keyed_events, submit_keyed_events,
stream_keyed_events): ONE keyed history written packed into a batch's pinned event slot, split by key and paired on the device, the
wire columns emitted straight into the batch's device stage.  Each such input, run, must be answered exactly as Batch.reload of the
host-split (columns.split_events), host-paired histories on a twin batch -- verdict, failing op, every counter -- by both search
kernels (lanes_per_history 8 and 64); two inputs in flight; every refusal (a malformed key, a key unfit for the wire format, too many
ops, more keys than the batch holds histories, no event) leaves the batch answering its resident input; a count-form batch refuses."""
import numpy as np
import pytest

import keyed_events_shapes as K
import pair_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns, core
from test_pair_events_gpu import KEYS, events_of
from test_submit_events_gpu import first_input, gm, opts

pytestmark = pytest.mark.gpu

key_of = lambda r: tuple(r[k] for k in KEYS)
answers = lambda batch: [key_of(r) for r in batch.run().results()]


def keyed(evs, seed):
    """the histories as ONE keyed history, round-robin, under scattered key values whose first rows are not in key order"""
    ks = (np.random.default_rng(seed).permutation(len(evs)) * 7919 - 200000).astype(np.int32)
    return K.interleave(evs, ks)


def host_split(ev, key):
    keys, ev_off, row_of = columns.split_events(ev, key)
    return keys, [columns.take_events(ev, row_of[int(ev_off[h]):int(ev_off[h + 1])]) for h in range(len(keys))]


@pytest.mark.parametrize("lanes", [8, 64])
def test_stream_keyed_events_equals_reload_of_host_split_histories(native, lanes):
    first = first_input()
    inputs = [keyed(events_of(300, 64, bad_every=4), 1), keyed(events_of(500, 57, n_ops=180), 2), keyed(events_of(700, 33, n_ops=150, bad_every=3), 3)]
    split = [host_split(ev, key) for ev, key in inputs]
    paired = [[columns.pair_events(e) for e in evs] for _, evs in split]
    with core.Batch(first, gm(), opts(lanes)) as by_keyed, core.Batch(first, gm(), opts(lanes)) as by_ops:
        by_keyed.run(), by_ops.run()
        by_keyed.map_events(0)          # (the event arena exists: what the first KEYED mapping adds is the split's own)
        bytes_before = native.lib().tbc_batch_device_bytes(by_keyed._h)
        m = by_keyed.map_keyed_events(0)
        assert native.lib().tbc_batch_device_bytes(by_keyed._h) - bytes_before >= 56 * m["events_cap"]          # the split's regions, counted
        assert m["events_cap"] == by_keyed.map_events(1)["events_cap"] and m["n_hist_cap"] == 64
        assert len(m["key"]) == len(m["ev_word"]) == len(m["process"]) == m["events_cap"]
        again = native.lib().tbc_batch_device_bytes(by_keyed._h)
        by_keyed.map_keyed_events(1)
        assert native.lib().tbc_batch_device_bytes(by_keyed._h) == again          # (once)
        for k in (0, 1):
            ev, key = inputs[k]
            by_ops.reload(paired[k])
            by_keyed.stream_keyed_events(ev, key, row_of=True)
            rep = by_keyed.events_report
            assert np.array_equal(rep["keys"], split[k][0]) and np.array_equal(rep["row_of"], columns.split_events(ev, key)[2])
            want, got = answers(by_ops), answers(by_keyed)
            assert len(got) == len(split[k][0]) == rep["n_keys"] and got == want, k
            assert {r[0] for r in got} >= {0, 1}
            info = by_keyed.input_info()
            assert info["total_ops"] == sum(len(h) for h in paired[k]) == rep["n_ops"] and info["pending"] == 0
            assert rep["bytes_in"] == 12 * len(ev) and info["bytes_copied"] == 12 * len(ev) + N.events_desc_bytes(rep["n_keys"])
            assert rep["n_bad"] == 0 and (rep["status"] == 0).all() and rep["ns_device"] > 0
        # two inputs in flight are consumed in order
        by_keyed.stream_keyed_events(*inputs[2]).stream_keyed_events(*inputs[0])
        assert by_keyed.input_info()["pending"] == 2
        by_ops.reload(paired[2])
        assert answers(by_keyed) == answers(by_ops)
        by_ops.reload(paired[0])
        assert answers(by_keyed) == answers(by_ops)
        # stream_events and stream_keyed_events on one batch: the slots, the arena and the stages are shared
        by_keyed.stream_events(split[1][1]).stream_keyed_events(*inputs[2])
        by_ops.reload(paired[1])
        assert answers(by_keyed) == answers(by_ops)
        by_ops.reload(paired[2])
        assert answers(by_keyed) == answers(by_ops)


def test_every_refusal_leaves_the_batch_answering_its_resident_input(native):
    good = events_of(500, 57, n_ops=180)
    with core.Batch(first_input(), gm(), opts(8)) as b:
        b.run()
        b.stream_keyed_events(*keyed(good, 4))
        resident = answers(b)
        info = b.input_info()

        def refused(ev, key, status):
            before = b.input_info()
            with pytest.raises(N.TbcError) as e:
                b.stream_keyed_events(ev, key)
            assert e.value.status == status, e.value.detail
            after = b.input_info()
            assert after["pending"] == 0 and after["inputs_consumed"] == before["inputs_consumed"] and after["total_ops"] == before["total_ops"]
            assert answers(b) == resident          # the resident input, answered once more
            return e.value

        # a malformed key among good ones: the report names the key's history and the row within the key's rows
        spoilt = list(good)
        spoilt[3] = S.cases()["malformed_each"][2]
        ev, key = keyed(spoilt, 5)
        h = list(columns.split_events(ev, key)[0]).index(int(key[np.flatnonzero(ev.process == 9)[-1]]))
        e = refused(ev, key, N.ERR_BAD_HISTORY)
        assert f"history {h}" in e.detail and "row 90" in e.detail
        assert e.report["n_bad"] == 1 and list(np.flatnonzero(e.report["status"])) == [h] and e.report["bad_row"][h] == 90
        # a surviving value the wire format does not hold
        unfit = list(good)
        unfit[5] = S.cases()["wire"][2]
        e = refused(*keyed(unfit, 6), N.ERR_UNSUPPORTED)
        assert e.report["n_bad"] == 1
        # more surviving ops than the batch's slots hold
        cap, ecap = info["ops_cap"], b.map_keyed_events(0)["events_cap"]
        many = events_of(900, 64, n_ops=int(cap) // 64 + 40, bad_every=0)
        n_ops = sum(len(columns.pair_events(x)) for x in many)
        assert n_ops > cap and sum(len(x) for x in many) <= ecap
        e = refused(*keyed(many, 7), N.ERR_INVALID_ARG)
        assert f"{n_ops} ops survive" in e.detail and e.report["n_ops"] == n_ops
        # more keys than the batch holds histories: decided from the number of keys alone
        ev, key = K.cases()["every_row_its_own_key"][0]
        e = refused(ev, key, N.ERR_INVALID_ARG)
        assert f"{len(key)} distinct keys" in e.detail and e.report["n_keys"] == len(key)
        e = refused(*keyed([S.H(S.pairs(4)) for _ in range(65)], 8), N.ERR_INVALID_ARG)
        assert "65 distinct keys" in e.detail
        # no event; more events than a slot holds
        lib, rep = native.lib(), N.KeyedReport()
        for n in (0, ecap + 1):
            assert lib.tbc_batch_submit_keyed_events(b._h, 0, n, rep) == N.ERR_INVALID_ARG and "a slot holds" in lib.tbc_last_error().decode()
        assert b.input_info()["pending"] == 0 and answers(b) == resident
        # exactly as many keys as the batch holds histories is fine
        b.stream_keyed_events(*keyed([S.H(S.pairs(6)) for _ in range(64)], 9))
        assert len(answers(b)) == 64


def test_slot_rules(native):
    lib = native.lib()
    ev, key = keyed(events_of(500, 20, n_ops=100), 10)
    with core.Batch(first_input(), gm(), opts(8)) as b:
        b.run()
        rep = N.KeyedReport()
        call = lambda slot, n: (lib.tbc_batch_submit_keyed_events(b._h, slot, n, rep), lib.tbc_last_error().decode())
        assert call(0, 1)[0] == N.ERR_INVALID_ARG and "never mapped" in call(0, 1)[1]
        b.map_events(0)                 # (mapped, but never for keyed events: the split's regions do not exist)
        assert call(0, 1)[0] == N.ERR_INVALID_ARG and "never mapped" in call(0, 1)[1]
        m = b.map_keyed_events(0)
        with pytest.raises(N.TbcError) as e:          # the first mapping of either kind fixed events_cap
            b.map_keyed_events(1, events_cap=m["events_cap"] + 1)
        assert e.value.status == N.ERR_INVALID_ARG
        with pytest.raises(N.TbcError):
            b.map_keyed_events(16)
        assert call(5, 1)[0] == N.ERR_INVALID_ARG
        b.stream_keyed_events(ev, key)          # (event slot 0)
        st, err = call(0, 20)
        assert st == N.ERR_INVALID_ARG and "still being copied" in err
        b.stream_keyed_events(ev, key)          # (event slot 1)
        st, err = call(1, 20)
        assert st == N.ERR_INVALID_ARG and "two inputs are waiting" in err
        first, second = answers(b), answers(b)
        assert first == second and len(first) == 20 and b.input_info()["pending"] == 0


def test_a_count_form_batch_refuses(native):
    first = first_input(info=0.03)
    ev, key = keyed(events_of(500, 57, n_ops=180, info=0.03), 11)
    with core.Batch(first, gm(), opts(8, count_form=True)) as b:
        b.run()
        with pytest.raises(N.TbcError) as e:
            b.map_keyed_events(0)
        assert e.value.status == N.ERR_UNSUPPORTED and "tbc_pair_events_batch" in e.value.detail
        st = native.lib().tbc_batch_submit_keyed_events(b._h, 0, 1, None)
        assert st == N.ERR_UNSUPPORTED and "tbc_pair_events_batch" in native.lib().tbc_last_error().decode()
        with pytest.raises(N.TbcError) as e:
            b.stream_keyed_events(ev, key)
        assert e.value.status == N.ERR_UNSUPPORTED
        resident = answers(b)
        assert answers(b) == resident

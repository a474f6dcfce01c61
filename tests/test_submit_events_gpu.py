"""tbc_batch_map_events / tbc_batch_submit_events on the MI355X (core.Batch.map_events, submit_events, stream_events): event histories
written packed into a batch's pinned event slot, paired on the device, their wire columns emitted straight into the batch's device
stage.  Each such input, run, must be answered exactly as Batch.reload of the host-paired columns on a twin batch -- verdict, failing
op, every counter -- by both search kernels (lanes_per_history 8 and 64); what crossed PCIe is 8 B an event and the descriptors; a
refused input (malformed, unfit for the wire format, too many ops) leaves the batch as it was; the slot rules; a count-form batch
refuses and keeps reload_events; reload_events and stream_events share one batch."""
import numpy as np
import pytest

import packed_events_shapes as P
import pair_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N, columns, core
from test_pair_events_gpu import KEYS, events_of

pytestmark = pytest.mark.gpu

key = lambda r: tuple(r[k] for k in KEYS)
keys = lambda batch: [key(r) for r in batch.run().results()]
gm = lambda: core.make_model(N.MODEL_CAS_REGISTER, N.NIL)


def opts(lanes, count_form=False):
    return core.make_opts(time_limit_ms=60000, algorithm=N.ALG_COMPETITION, want_witness=False, count_form=count_form, lanes_per_history=lanes,
                          search_width=4 if lanes == 64 and not count_form else 0)


def first_input(info=0.0):
    return [columns.pair_events(e) for e in events_of(100, 64, info=info)]


def copied(evs):
    return 8 * sum(len(e) for e in evs) + 8 * (len(evs) + 1) + P.descriptor_bytes(len(evs))


@pytest.mark.parametrize("lanes", [8, 64])
def test_stream_events_equals_reload_of_host_paired_columns(native, lanes):
    first = first_input()
    inputs = [events_of(300, 64, bad_every=4), events_of(500, 57, n_ops=180), events_of(700, 33, n_ops=150, bad_every=3)]
    paired = [[columns.pair_events(e) for e in evs] for evs in inputs]
    with core.Batch(first, gm(), opts(lanes)) as by_events, core.Batch(first, gm(), opts(lanes)) as by_ops:
        by_events.run(), by_ops.run()
        by_events.map_input(0)          # (the streaming side of the batch exists: what the first mapping of events adds is its own)
        before, bytes_before = by_events.input_info(), native.lib().tbc_batch_device_bytes(by_events._h)
        m = by_events.map_events(0)
        assert native.lib().tbc_batch_device_bytes(by_events._h) - bytes_before >= 24 * m["events_cap"]          # the device event arena, counted
        assert m["events_cap"] == 3 * before["ops_cap"] and m["n_hist_cap"] == before["n_hist_cap"] == 64
        assert len(m["ev_word"]) == len(m["process"]) == m["events_cap"] and len(m["ev_off"]) == 65
        # two successive inputs, each run
        for k in (0, 1):
            by_ops.reload(paired[k])
            by_events.stream_events(inputs[k])
            want, got = keys(by_ops), keys(by_events)
            assert len(got) == len(inputs[k]) and got == want, k
            assert {r[0] for r in got} >= {0, 1}
            info = by_events.input_info()
            assert info["total_ops"] == sum(len(h) for h in paired[k]) == by_events.events_report["n_ops"]
            assert info["bytes_copied"] == copied(inputs[k]) and info["pending"] == 0
            assert by_events.events_report["bytes_in"] == 8 * sum(len(e) for e in inputs[k]) + 8 * (len(inputs[k]) + 1)
            assert by_events.events_report["n_bad"] == 0 and (by_events.events_report["status"] == 0).all() and by_events.events_report["ns_device"] > 0
        # two inputs submitted before one run are consumed in order
        by_events.stream_events(inputs[2]).stream_events(inputs[0])
        assert by_events.input_info()["pending"] == 2
        by_ops.reload(paired[2])
        assert keys(by_events) == keys(by_ops) and by_events.input_info()["bytes_copied"] == copied(inputs[2])
        by_ops.reload(paired[0])
        assert keys(by_events) == keys(by_ops) and by_events.input_info()["bytes_copied"] == copied(inputs[0])
        # reload_events and stream_events on one batch: the stages and their order are shared
        by_events.reload_events(inputs[1]).stream_events(inputs[2])
        by_ops.reload(paired[1])
        assert keys(by_events) == keys(by_ops) and by_events.input_info()["bytes_copied"] == 12 * sum(len(h) for h in paired[1])
        by_ops.reload(paired[2])
        assert keys(by_events) == keys(by_ops)
        by_events.stream_events(inputs[0]).reload_events(inputs[1])
        by_ops.reload(paired[0])
        assert keys(by_events) == keys(by_ops)
        by_ops.reload(paired[1])
        assert keys(by_events) == keys(by_ops)


def test_a_refused_input_leaves_the_batch_as_it_was(native):
    good = events_of(500, 57, n_ops=180)
    with core.Batch(first_input(), gm(), opts(8)) as b:
        b.run()
        b.stream_events(good)
        resident = keys(b)
        info = b.input_info()

        def refused(evs, status):
            before = b.input_info()
            with pytest.raises(N.TbcError) as e:
                b.stream_events(evs)
            assert e.value.status == status, e.value.detail
            after = b.input_info()
            assert after["pending"] == 0 and after["inputs_consumed"] == before["inputs_consumed"] and after["total_ops"] == before["total_ops"]
            assert keys(b) == resident          # the resident input, answered once more
            return e.value

        # a malformed history among good ones: the report names the history and the row
        spoilt = list(good)
        spoilt[3] = S.cases()["malformed_each"][2]
        e = refused(spoilt, N.ERR_BAD_HISTORY)
        assert "history 3" in e.detail and "row 90" in e.detail
        assert e.report["n_bad"] == 1 and list(np.flatnonzero(e.report["status"])) == [3] and e.report["status"][3] == N.ERR_BAD_HISTORY and e.report["bad_row"][3] == 90
        assert (np.delete(e.report["bad_row"], 3) == N.PAIR_NO_ROW).all()
        # a surviving value the wire format does not hold (and, behind it, a malformed history: malformed wins)
        unfit = list(good)
        unfit[5] = S.cases()["wire"][2]
        e = refused(unfit, N.ERR_UNSUPPORTED)
        assert "history 5" in e.detail and e.report["status"][5] == N.ERR_UNSUPPORTED and e.report["n_bad"] == 1
        unfit[9] = S.cases()["malformed_each"][0]
        e = refused(unfit, N.ERR_BAD_HISTORY)
        assert "history 9" in e.detail and "row 91" in e.detail and e.report["n_bad"] == 2
        # a failed op with such a value is fine
        held = list(good)
        held[5] = S.H([(S.I, 0, S.W, 255, 0), (S.FAIL, 0, S.W, 255, 0), (S.I, 0, S.CAS, 1, -7), (S.FAIL, 0, S.CAS, 1, -7), (S.I, 0, S.W, 1, 0), (S.OK, 0, S.W, 1, 0)])
        b.stream_events(held)
        assert len(keys(b)) == len(held)
        b.stream_events(good)
        assert keys(b) == resident
        # more surviving ops than the batch's slots hold
        cap, ecap = info["ops_cap"], b.map_events(0)["events_cap"]
        many = events_of(900, 64, n_ops=int(cap) // 64 + 40, bad_every=0)
        n_ops = sum(len(columns.pair_events(x)) for x in many)
        assert n_ops > cap and sum(len(x) for x in many) <= ecap
        e = refused(many, N.ERR_INVALID_ARG)
        assert f"{n_ops} ops survive" in e.detail and e.report["n_ops"] == n_ops


def test_slot_rules(native):
    lib = native.lib()
    good = events_of(500, 20, n_ops=100)
    with core.Batch(first_input(), gm(), opts(8)) as b:
        b.run()
        rep = N.EventsReport()
        call = lambda slot, n: (lib.tbc_batch_submit_events(b._h, slot, n, rep), lib.tbc_last_error().decode())
        st, err = call(0, 1)          # nothing mapped at all
        assert st == N.ERR_INVALID_ARG and "never mapped" in err
        m = b.map_events(0)
        with pytest.raises(N.TbcError) as e:          # the first mapping fixed events_cap
            b.map_events(1, events_cap=m["events_cap"] + 1)
        assert e.value.status == N.ERR_INVALID_ARG
        assert b.map_events(1, events_cap=100)["events_cap"] == m["events_cap"]
        with pytest.raises(N.TbcError):
            b.map_events(16)
        st, err = call(5, 1)
        assert st == N.ERR_INVALID_ARG and "never mapped" in err
        assert call(0, 0)[0] == N.ERR_INVALID_ARG and call(0, 65)[0] == N.ERR_INVALID_ARG
        m["ev_off"][:3] = [0, 10, 5]
        st, err = call(0, 2)
        assert st == N.ERR_INVALID_ARG and "descends" in err
        m["ev_off"][:2] = [0, m["events_cap"] + 1]
        st, err = call(0, 1)
        assert st == N.ERR_INVALID_ARG and "a slot holds" in err
        assert b.input_info()["pending"] == 0
        # a slot submitted while its events are still the device's to read
        b.stream_events(good)          # (event slot 0)
        st, err = call(0, 20)
        assert st == N.ERR_INVALID_ARG and "still being copied" in err
        b.stream_events(good)          # (event slot 1)
        st, err = call(1, 20)          # a third pending input
        assert st == N.ERR_INVALID_ARG and "two inputs are waiting" in err
        first, second = keys(b), keys(b)
        assert first == second and len(first) == 20 and b.input_info()["pending"] == 0


def test_a_count_form_batch_refuses_and_keeps_reload_events(native):
    first = first_input(info=0.03)
    evs = events_of(500, 57, n_ops=180, info=0.03)
    with core.Batch(first, gm(), opts(8, count_form=True)) as b, core.Batch(first, gm(), opts(8, count_form=True)) as by_ops:
        b.run(), by_ops.run()
        with pytest.raises(N.TbcError) as e:
            b.map_events(0)
        assert e.value.status == N.ERR_UNSUPPORTED and "tbc_pair_events_batch" in e.value.detail
        st = native.lib().tbc_batch_submit_events(b._h, 0, 1, None)
        assert st == N.ERR_UNSUPPORTED and "tbc_pair_events_batch" in native.lib().tbc_last_error().decode()
        with pytest.raises(N.TbcError) as e:
            b.stream_events(evs)
        assert e.value.status == N.ERR_UNSUPPORTED
        b.reload_events(evs)
        by_ops.reload([columns.pair_events(x) for x in evs])
        assert keys(b) == keys(by_ops)

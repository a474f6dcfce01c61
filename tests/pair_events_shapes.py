"""The event histories tbc_pair_events_batch is tested on, shared by the emulator test (tests/test_pair_events_emu.py) and the GPU test
(tests/test_pair_events_gpu.py): the smallest shapes at which each mechanism of csrc/pair_kernels.h can go wrong -- chunk edges of 64
events, the process table (4,096 entries, ids folded to 12 bits by pr::table_hash), the semantics of tbc_pair_events, each malformed
row -- and the reference: tbc_pair_events itself, history by history (pinned by tests/test_host_logic.py).  A case is a BATCH: a list
of histories that go into one call."""
import re

import numpy as np

from jepsen_tigerbeetle_amd import _native as N, columns
from jepsen_tigerbeetle_amd.columns import EventColumns

I, OK, FAIL, INFO = N.INVOKE, N.OK, N.FAIL, N.INFO
R, W, CAS = N.F_READ, N.F_WRITE, N.F_CAS
NIL = N.NIL
TABLE = N.PAIR_MAX_PROCESS


def table_hash(k):
    """pr::table_hash of csrc/pair_plan.h (the emulator test holds it against the C function)"""
    k &= 0xFFFFFFFF
    return (k ^ (k >> 12) ^ (k >> 24)) & (TABLE - 1)


def H(rows):
    """rows of (type, process, f, a, b) -> EventColumns"""
    a = np.array(rows, np.int64).reshape(-1, 5)
    return EventColumns(a[:, 0].astype(np.uint8), a[:, 1].astype(np.int32), a[:, 2].astype(np.uint8), a[:, 3].astype(np.int32), a[:, 4].astype(np.int32))


def pairs(n_events, procs=(0, 1, 2), f=W, base=0):
    """a well-formed history of exactly n_events rows: the processes take turns to invoke and complete :ok; an odd row count ends
    on an invocation that never completes"""
    rows = []
    k = 0
    while len(rows) < n_events:
        p = procs[k % len(procs)]
        rows.append((I, p, f, (base + k) % 5, 0))
        if len(rows) < n_events:
            rows.append((OK, p, f, (base + k) % 5, 0))
        k += 1
    return rows


def _cases():
    c = {}
    c["lengths"] = [H(pairs(n)) for n in (0, 1, 2, 63, 64, 65, 128, 129)] + [H(pairs(64 * 70 + 5, procs=tuple(range(7))))]
    # an invocation in lane 63, its completion in lane 0 of the next chunk; the same one chunk later with the values learnt
    edge = pairs(62) + [(I, 100, W, 1, 0), (I, 7, R, NIL, 0), (OK, 7, R, 3, 0), (OK, 100, W, 1, 0)]
    edge2 = pairs(126, procs=(0, 1)) + [(I, 100, W, 1, 0), (I, 7, CAS, 1, 2), (FAIL, 7, CAS, 1, 2), (I, 7, R, NIL, 0)] + pairs(70) + [(OK, 7, R, 4, 0)]
    # a process silent for many chunks, then completing (:ok, :fail, :info), and one that never does
    silent = [(I, 50, R, NIL, 0), (I, 51, W, 2, 0), (I, 52, W, 3, 0), (I, 53, W, 4, 0)] + pairs(64 * 9 + 17) + [(OK, 50, R, 2, 0), (FAIL, 51, W, 2, 0), (INFO, 52, W, 3, 0)]
    c["chunk_edges"] = [H(edge), H(edge2), H(silent)]
    many = lambda n, ids=None: H([x for p in (ids if ids is not None else range(n)) for x in ((I, p, W, p % 5, 0),)] +
                                 [x for p in (ids if ids is not None else range(n)) for x in ((OK, p, W, p % 5, 0),)])
    c["processes_1_64_65"] = [many(1), many(64), many(65), H(pairs(200, procs=tuple(range(65))))]
    c["processes_4096_and_4097"] = [many(4096), many(4097), H(pairs(10)), many(4096, ids=[NIL] + list(range(4095))), many(4097, ids=[NIL] + list(range(4096)))]
    # which refusal wins (include/tbcheck.h): ids are counted in steps of 64 rows up to and including the step of the first malformed row
    # -- there more than 4,096 is UNSUPPORTED, past it the history is malformed; rows of an unknown type carry no id
    inv = lambda ids: [(I, p, W, p % 5, 0) for p in ids]
    oks = lambda ids: [(OK, p, W, p % 5, 0) for p in ids]
    c["refusal_precedence"] = [
        H([(OK, 9, W, 1, 0)] + inv(range(100, 4197)) + oks(range(100, 4197))),         # malformed in step 0, 4,097 ids after it: malformed, row 0
        H(inv(range(4097)) + oks(range(4097)) + [(OK, 99999, W, 1, 0)]),               # 4,097 ids, a malformed row behind them: unsupported
        H(inv(range(4096)) + [(7, 5000, W, 0, 0)]),                                    # the 4,097th id on a row of unknown type: malformed
        H(inv(range(4096)) + [(OK, 77777, W, 1, 0)]),                                  # the 4,097th id IS the malformed row (one step): unsupported
        H(inv(range(4096)) + [(I, 5, W, 1, 0)] + inv(range(5000, 5010))),              # malformed (id 5 is open), new ids behind it in its step: they count, unsupported
        H(inv(range(4096)) + oks(range(64)) + [(I, 100, W, 1, 0)] + oks(range(64, 127)) + inv(range(6000, 6100))),   # 4,096 ids, malformed, more ids in later steps: malformed
    ]
    c["process_ids"] = [
        H(pairs(150, procs=(-1, -2, -2 ** 31, 2 ** 31 - 1, -4096, 0))),
        # ids that collide in the table: equal modulo its size (1, 4097, 8193 -- and 4097 folds onto 0), equal after the fold (1, 4096, 1 << 24)
        H(pairs(300, procs=(1, 4097, 8193, 0, 4096, 1 << 24, (1 << 24) + 4096, 1 + 4096 * 4097))),
        H(pairs(40, procs=(4096, 1))), H(pairs(40, procs=(1, 4096))),
    ]
    # Jepsen's numbering: a process that crashes comes back as p + concurrency
    conc, rows, ids = 5, [], list(range(5))
    for k in range(120):
        w = k % conc
        rows.append((I, ids[w], W, k % 5, 0))
        if k % 7 == 3:
            rows.append((INFO, ids[w], W, k % 5, 0))
            ids[w] += conc
        else:
            rows.append((OK if k % 4 else FAIL, ids[w], W, k % 5, 0))
    c["jepsen_renumbering"] = [H(rows), H(rows[:77])]
    c["semantics"] = [
        H([(I, 0, R, NIL, 0), (I, 1, CAS, 1, 2), (OK, 0, R, 4, 9), (OK, 1, CAS, 3, 4)]),                 # :ok values override; a nil read learns its value
        H([(I, 0, W, 1, 0), (FAIL, 0, W, 1, 0), (I, 0, W, 2, 0), (FAIL, 0, W, 2, 0), (I, 0, W, 3, 0), (OK, 0, W, 3, 0)]),   # adjacent fails
        H([x for k in range(40) for x in ((I, k % 3, W, k % 5, 0), ((FAIL, OK)[k % 2], k % 3, W, k % 5, 0))]),     # alternating
        H([x for k in range(70) for x in ((I, k % 4, W, 1, 0), (FAIL, k % 4, W, 1, 0))]),                 # all :fail: no op, no process
        # process 5's first op fails and a later one survives: its dense number is not its first appearance among the events
        H([(I, 5, W, 1, 0), (I, 6, W, 2, 0), (FAIL, 5, W, 1, 0), (OK, 6, W, 2, 0), (I, 7, W, 3, 0), (I, 5, W, 4, 0), (OK, 5, W, 4, 0), (OK, 7, W, 3, 0)]),
        H([(I, 0, W, 1, 0), (INFO, 0, W, 1, 0), (I, 1, R, NIL, 0), (INFO, 1, R, 3, 0), (I, 2, W, 2, 0), (OK, 2, W, 2, 0)]),    # :info: crashed, the invocation's values
        H([(I, 0, W, 1, 0), (I, 1, W, 2, 0), (OK, 1, W, 2, 0), (I, 2, R, NIL, 0)]),                       # never completed
        H([(I, p, W, p % 5, 0) for p in range(70)]),                                                      # invocations only
        # the same across chunk edges: a failing first op and the survivor in different chunks, other processes first seen in between
        H([(I, 5, W, 1, 0), (FAIL, 5, W, 1, 0)] + pairs(100, procs=(6, 7)) + [(I, 5, W, 4, 0)] + pairs(64, procs=(8,)) + [(OK, 5, W, 4, 0)]),
    ]
    good = pairs(90)
    c["malformed_each"] = [
        H(good + [(I, 0, W, 1, 0), (I, 0, W, 2, 0)]),                      # an invocation while an op is open
        H(good + [(I, 0, W, 1, 0), (INFO, 0, W, 1, 0), (I, 0, W, 2, 0)]),  # an invocation after an :info
        H(good + [(OK, 9, W, 1, 0)]),                                      # a completion without an invocation
        H(good + [(7, 0, W, 1, 0)]),                                       # an unknown type code
        H([(OK, 0, W, 1, 0)] + good),                                      # an error in row 0 ...
        H([(4, 0, W, 1, 0)] + good),
        H(good + [(I, 0, W, 1, 0), (INFO, 0, W, 1, 0), (OK, 0, W, 1, 0)]),  # an :info followed by a completion of the same process
        H(good + [(I, 0, W, 1, 0), (OK, 0, W, 1, 0), (FAIL, 0, W, 1, 0)]),  # a second completion
    ]
    # two errors in different chunks (the lower row is reported), in both orders of kind; two in one chunk; an error in lane 63 and in lane 0
    c["malformed_two"] = [
        H(pairs(70) + [(OK, 9, W, 1, 0)] + pairs(130) + [(I, 0, W, 1, 0), (I, 0, W, 1, 0)]),
        H(pairs(70) + [(I, 0, W, 1, 0), (I, 0, W, 1, 0), (OK, 0, W, 1, 0)] + pairs(130) + [(9, 0, W, 1, 0)]),
        H(pairs(10) + [(9, 0, W, 1, 0), (OK, 9, W, 1, 0)] + pairs(10)),
        H(pairs(63, procs=(0, 1)) + [(OK, 9, W, 1, 0)] + pairs(10, procs=(2, 3))),
        H(pairs(64) + [(OK, 9, W, 1, 0)] + pairs(10)),
        # open across a chunk edge, invoked again in the next chunk
        H(pairs(62) + [(I, 7, W, 1, 0)] + pairs(66, procs=(0, 1)) + [(I, 7, W, 2, 0)]),
    ]
    bad = H(pairs(20) + [(OK, 9, W, 1, 0)])
    c["bad_among_good"] = [bad, H(pairs(100)), H(pairs(65)), bad, H(pairs(3)), H(pairs(129)), H([(5, 1, W, 0, 0)])]
    c["wire"] = [
        H(pairs(100)),
        H([(I, 0, R, NIL, 0), (OK, 0, R, 254, 0), (I, 1, CAS, 0, 254), (OK, 1, CAS, NIL, NIL), (I, 2, W, 7, 300), (OK, 2, W, 7, -5)]),   # b out of range outside :cas: ignored
        H([(I, 0, W, 255, 0), (OK, 0, W, 255, 0)]),                        # a value of 255
        H([(I, 0, 16, 1, 0), (OK, 0, 16, 1, 0)]),                          # an :f of 16
        H([(I, 0, CAS, 1, 255), (OK, 0, CAS, 1, 255)]),                    # :cas with b out of range
        H([(I, 0, W, 255, 0), (FAIL, 0, W, 255, 0), (I, 0, W, 1, 0)]),     # ... in an op that does not survive: held
        H([(I, 0, R, 300, 0), (OK, 0, R, 3, 0), (I, 0, 15, -7, 0), (OK, 0, 15, 254, 0)]),   # the completion's value is what counts
        H([(I, 0, W, -1, 0)]),
    ]
    return c


WORD_CASES = ("wire", "lengths", "semantics", "processes_4096_and_4097", "bad_among_good", "refusal_precedence")
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def random_batch():
    """200 seeded synth.register_events histories of 50..400 ops, the :info and :fail (corrupt cas) rates varied"""
    from jepsen_tigerbeetle_amd import synth
    rng = np.random.default_rng(2024)
    out = []
    for s in range(200):
        out.append(synth.register_events(n_ops=int(rng.integers(50, 401)), n_procs=int(rng.integers(1, 40)), seed=1000 + s, busy=float(rng.choice([0.1, 0.5, 0.9])),
                                         info=float(rng.choice([0.0, 0.01, 0.05, 0.2])), read=float(rng.choice([0.1, 1 / 3])), write=float(rng.choice([0.1, 1 / 3]))))
    return out


_REFS = {}


def wire_reference(ops):
    """TBC_WIRE_WORD of host-paired columns as tbc_batch_reload encodes it (csrc/batch_stream.hip): None if the wire format does not
    hold them -- f 0..15, a 0..254 or nil, b likewise for :cas (elsewhere an out-of-range b travels as 0), process 0..4095"""
    f, a, b, p = (ops.f.astype(np.int64), ops.a.astype(np.int64), ops.b.astype(np.int64), ops.process.astype(np.int64))
    a_ok = (a == NIL) | ((a >= 0) & (a <= 254))
    b_ok = (b == NIL) | ((b >= 0) & (b <= 254))
    if ((f > 15) | ~a_ok | ((f == CAS) & ~b_ok) | (p < 0) | (p > 4095)).any():
        return None
    a8 = np.where(a == NIL, N.WIRE_NIL, a)
    b8 = np.where(~b_ok, 0, np.where(b == NIL, N.WIRE_NIL, b))
    return (f | (a8 << 4) | (b8 << 12) | (p << 20)).astype(np.uint32)


def reference(name, evs, word):
    """What tbc_pair_events_batch must give for the batch: tbc_pair_events history by history (computed once per case and kept)."""
    key = (name, word)
    if key in _REFS:
        return _REFS[key]
    nh = len(evs)
    want = {"status": np.zeros(nh, np.int32), "bad_row": np.full(nh, N.PAIR_NO_ROW, np.uint32), "n_events": np.array([len(e) for e in evs], np.uint32),
            "n_process": np.zeros(nh, np.uint32), "op_off": np.zeros(nh + 1, np.uint64)}
    cols = {k: [] for k in ("f", "a", "b", "process", "inv_pos", "ret_pos", "word")}
    for h, e in enumerate(evs):
        ops, bad = None, None
        try:
            ops = columns.pair_events(e)
        except N.TbcError as err:
            assert err.status == N.ERR_BAD_HISTORY
            bad = int(re.match(r"row (\d+):", err.detail).group(1))
        # the documented precedence: the ids of the rows of a known type, up to the end of the 64-row step of the first malformed row
        upto = len(e) if bad is None else 64 * (bad // 64 + 1)
        if len(np.unique(e.process[:upto][e.type[:upto] <= INFO])) > TABLE:
            want["status"][h], ops = N.ERR_UNSUPPORTED, None
        elif bad is not None:
            want["status"][h], want["bad_row"][h] = N.ERR_BAD_HISTORY, bad
        if ops is not None and word and len(ops):
            w = wire_reference(ops)
            if w is None:
                want["status"][h] = N.ERR_UNSUPPORTED
                ops = None
            else:
                cols["word"].append(w)
        if ops is not None:
            want["n_process"][h] = ops.n_process
            for k in ("f", "a", "b", "process", "inv_pos", "ret_pos"):
                cols[k].append(getattr(ops, k))
        want["op_off"][h + 1] = want["op_off"][h] + (len(ops) if ops is not None else 0)
    dt = {"f": np.uint8, "a": np.int32, "b": np.int32, "process": np.int32, "inv_pos": np.uint32, "ret_pos": np.uint32, "word": np.uint32}
    for k, v in cols.items():
        if k != "word" or word:
            want[k] = np.concatenate(v).astype(dt[k]) if v else np.zeros(0, dt[k])
    want["n_ops"] = int(want["op_off"][-1])
    want["n_bad"] = int((want["status"] != 0).sum())
    _REFS[key] = want
    return want


def assert_same(got, want, what):
    """every array bit for bit: the descriptors whole, the op arrays up to the total"""
    T = want["n_ops"]
    assert (got["n_ops"], got["n_bad"]) == (T, want["n_bad"]), (what, got["n_ops"], got["n_bad"], T, want["n_bad"])
    for k in ("status", "bad_row", "op_off"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    nh = len(want["status"])
    for k in ("n_events", "n_process"):
        assert np.array_equal(got[k][:nh], want[k]), (what, k, got[k][:nh], want[k])
    for k in ("f", "a", "b", "process", "inv_pos", "ret_pos", "word"):
        if k in want:
            assert k in got, (what, k)
            if not np.array_equal(got[k][:T], want[k]):
                at = int(np.flatnonzero(got[k][:T] != want[k])[0])
                raise AssertionError((what, k, "first difference at op", at, int(got[k][at]), int(want[k][at])))


def structs(ev_off, ev, ops_cap, arrays):
    """tbc_event_batch and tbc_pair_out over the caller's own op arrays (`arrays`: name -> numpy array; the descriptors are made here)
    -> (in, out, what must stay alive)"""
    import ctypes as C
    p = columns._p
    nh = len(ev_off) - 1
    keep = {"op_off": np.zeros(nh + 1, np.uint64), "n_events": np.zeros(max(nh, 1), np.uint32), "n_process": np.zeros(max(nh, 1), np.uint32),
            "status": np.zeros(max(nh, 1), np.int32), "bad_row": np.zeros(max(nh, 1), np.uint32)}
    keep.update(arrays)
    i = N.EventBatch()
    i.n_hist, i.device, i.ev_off = nh, 0, p(ev_off, C.c_uint64)
    i.type, i.process, i.f, i.a, i.b = p(ev.type, C.c_uint8), p(ev.process, C.c_int32), p(ev.f, C.c_uint8), p(ev.a, C.c_int32), p(ev.b, C.c_int32)
    o = N.PairOut()
    o.ops_cap = ops_cap
    ct = {"op_off": C.c_uint64, "n_events": C.c_uint32, "n_process": C.c_uint32, "f": C.c_uint8, "a": C.c_int32, "b": C.c_int32, "process": C.c_int32,
          "inv_pos": C.c_uint32, "ret_pos": C.c_uint32, "word": C.c_uint32, "status": C.c_int32, "bad_row": C.c_uint32}
    for k, v in keep.items():
        setattr(o, k, p(v, ct[k]))
    return i, o, keep

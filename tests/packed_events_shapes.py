"""The packed event word of include/tbcheck.h (TBC_EVENT_WORD: 8 B an event with the process column, instead of 14) stated in numpy --
the encoding tbc_pack_events must give, its decoding, and what the packed reader of csrc/pair_kernels.h must answer: tbc_pair_events
over the DECODED events, history by history (tests/pair_events_shapes.py's reference with the wire word asked for, as a batch asks).
The codes "a type that is none of the four", "an :f above 15" and "a value the wire format does not hold" decode to one value of
their class each (7, 16, 256), so every rule of the pairing decides the decoded history as it decides the original.  Beside the
shapes of pair_events_shapes.py, the histories here put every edge of the four fields on a surviving op, a failed op and a crashed
op, each as one history among good ones."""
import numpy as np

import pair_events_shapes as S
from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.columns import EventColumns

I, OK, FAIL, INFO, R, W, CAS, NIL = S.I, S.OK, S.FAIL, S.INFO, S.R, S.W, S.CAS, S.NIL
TYPE_UNKNOWN, F_ABOVE, V_NIL, V_UNFIT = 7, 16, 255, 256


def event_word(type, f, a, b):
    """TBC_EVENT_WORD over ENCODED fields: type bits 0-2, f bits 3-7, a bits 8-16, b bits 17-25"""
    u = lambda x: np.asarray(x).astype(np.uint32)
    return u(type) | (u(f) << np.uint32(3)) | (u(a) << np.uint32(8)) | (u(b) << np.uint32(17))


def encode_value(v):
    v = np.asarray(v).astype(np.int64)
    return np.where(v == NIL, V_NIL, np.where((v >= 0) & (v <= 254), v, V_UNFIT))


def pack(e):
    """one history's columns -> its words (the process column travels as it is)"""
    t, f = e.type.astype(np.int64), e.f.astype(np.int64)
    return event_word(np.where(t <= INFO, t, TYPE_UNKNOWN), np.where(f <= 15, f, F_ABOVE), encode_value(e.a), encode_value(e.b)).astype(np.uint32)


def decode(words, process):
    w = np.asarray(words).astype(np.int64)
    val = lambda x: np.where(x == V_NIL, NIL, x).astype(np.int32)
    return EventColumns((w & 7).astype(np.uint8), np.asarray(process).astype(np.int32), ((w >> 3) & 31).astype(np.uint8), val((w >> 8) & 511), val((w >> 17) & 511))


def decoded(evs):
    return [decode(pack(e), e.process) for e in evs]


def _field_edges():
    """every edge of f, a and b on an op that survives (:ok), one that fails and one that crashes (:info), a good history in between"""
    out = []
    variants = [(f, 1, 0) for f in (15, 16, 255)] + [(W, a, 0) for a in (254, 255, 256, -1, NIL)] + \
               [(f, 1, b) for f in (CAS, W) for b in (254, 255, 256, -1, NIL)]
    for done in (OK, FAIL, INFO):
        for k, (f, a, b) in enumerate(variants):
            if k % 6 == 0:
                out.append(S.H(S.pairs(30 + k)))
            out.append(S.H(S.pairs(10) + [(I, 9, f, a, b), (done, 9, f, a, b)] + S.pairs(7)))
    return out


def _cases():
    c = dict(S.cases())
    good = lambda n: S.H(S.pairs(n))
    c["packed_type_codes"] = [good(20), S.H(S.pairs(12) + [(4, 0, W, 1, 0)] + S.pairs(4)), good(65), S.H(S.pairs(70) + [(255, 3, W, 1, 0)]), good(3),
                              S.H(S.pairs(5) + [(5, 0, W, 1, 0)]), S.H(S.pairs(5) + [(6, 0, W, 1, 0)])]
    c["packed_field_edges"] = _field_edges()
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def packed_reference(name, evs):
    """tbc_pair_events over the decoded events, the wire word asked for (computed once per case and kept)"""
    return S.reference("packed/" + name, decoded(evs), True)


def concat_packed(evs):
    """(ev_off u64[n + 1], ev_word u32[events], process i32[events]) of the histories side by side"""
    nh = len(evs)
    ev_off = np.zeros(nh + 1, np.uint64)
    if nh:
        np.cumsum(np.fromiter((len(e) for e in evs), np.uint64, nh), out=ev_off[1:])
    words = np.concatenate([pack(e) for e in evs]).astype(np.uint32) if nh else np.zeros(0, np.uint32)
    process = np.ascontiguousarray(np.concatenate([e.process for e in evs]).astype(np.int32)) if nh else np.zeros(0, np.int32)
    return ev_off, np.ascontiguousarray(words), process


def descriptor_bytes(n_hist):
    """what tbc_batch_submit_events brings back: the accumulator (16 B), op_off, and n_events, n_process, status, bad_row: 24 B a history"""
    return 16 + 8 * (n_hist + 1) + 16 * n_hist

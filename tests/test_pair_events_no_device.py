"""tbc_pair_events_batch without a device: the arguments are held against the rules of the struct BEFORE the device is looked for --
a null argument, an ev_off that does not start at 0 or descends, too many rows are TBC_ERR_INVALID_ARG on any machine -- and valid
input on a machine without a gfx950 is TBC_ERR_NO_DEVICE: there is no CPU fallback.  (tests/test_abi.py holds the symbol and its
binding; the struct layouts are held against the header here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pair_events_shapes as S
from conftest import ROOT, has_gpu
from jepsen_tigerbeetle_amd import _native as N, columns


def call(native, i, o):
    st = native.lib().tbc_pair_events_batch(C.byref(i) if i is not None else None, C.byref(o) if o is not None else None)
    return st, native.lib().tbc_last_error().decode()


def make(evs, ops_cap=None):
    ev_off, ev = columns.concat_events(evs)
    n = int(ev_off[-1])
    arrays = {k: np.zeros(max(n, 1), dt) for k, dt in (("inv_pos", np.uint32), ("ret_pos", np.uint32))}
    return S.structs(ev_off, ev, n if ops_cap is None else ops_cap, arrays) + (ev_off, ev)


def test_arguments_are_validated_first(native):
    evs = S.cases()["semantics"]
    assert call(native, None, None)[0] == N.ERR_INVALID_ARG
    i, o, keep, ev_off, ev = make(evs)
    assert call(native, i, None)[0] == N.ERR_INVALID_ARG and call(native, None, o)[0] == N.ERR_INVALID_ARG
    for field in ("ev_off", "type", "process", "f", "a", "b"):
        i, o, keep, ev_off, ev = make(evs)
        setattr(i, field, None)
        st, err = call(native, i, o)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    for field in ("op_off", "n_events", "n_process", "status", "bad_row", "inv_pos", "ret_pos"):
        i, o, keep, ev_off, ev = make(evs)
        setattr(o, field, None)
        st, err = call(native, i, o)
        assert st == N.ERR_INVALID_ARG and "null argument" in err, (field, err)
    i, o, keep, ev_off, ev = make(evs)
    ev_off[0] = 1
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "ev_off[0]" in err
    i, o, keep, ev_off, ev = make(evs)
    ev_off[3] = ev_off[2] - 1
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "history 2" in err and "descends" in err
    # sizes alone decide these: no event is looked at
    i, o, keep, ev_off, ev = make(evs)
    ev_off[1:] += np.uint64(1 << 31)
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "history 0 has 2^31 events" in err
    i, o, keep, ev_off, ev = make(evs)
    ev_off[1:] = (np.arange(1, len(ev_off)) * ((1 << 31) - 1)).astype(np.uint64)
    st, err = call(native, i, o)
    assert st == N.ERR_INVALID_ARG and "2^32 - 1 events" in err


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback(native):
    i, o, keep, ev_off, ev = make(S.cases()["semantics"])
    assert call(native, i, o)[0] == N.ERR_NO_DEVICE
    with pytest.raises(N.NoDeviceError):
        columns.pair_events_batch(S.cases()["semantics"])
    i, o, keep, ev_off, ev = make([])
    assert call(native, i, o)[0] == N.ERR_NO_DEVICE


def test_struct_layouts_match_header(native):
    prog = r'''
#include <stdio.h>
#include "tbcheck.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u\n", sizeof(tbc_event_batch), offsetof(tbc_event_batch, ev_off),
  offsetof(tbc_event_batch, b), sizeof(tbc_pair_out), offsetof(tbc_pair_out, op_off), offsetof(tbc_pair_out, f), offsetof(tbc_pair_out, word),
  offsetof(tbc_pair_out, status), offsetof(tbc_pair_out, n_bad), offsetof(tbc_pair_out, n_ops), offsetof(tbc_pair_out, bytes_in),
  TBC_PAIR_MAX_PROCESS, TBC_PAIR_NO_ROW); return 0; }
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    E, P = N.EventBatch, N.PairOut
    assert sizes == [C.sizeof(E), E.ev_off.offset, E.b.offset, C.sizeof(P), P.op_off.offset, P.f.offset, P.word.offset, P.status.offset,
                     P.n_bad.offset, P.n_ops.offset, P.bytes_in.offset, N.PAIR_MAX_PROCESS, N.PAIR_NO_ROW]
    assert native.lib().tbc_version() == 2


def test_the_shim_binds_the_entry_point_by_its_own_table(native):
    """clj/src/tigerbeetle/checker/gpu_linear.clj: `pair-abi` -- the two structs of tbc_pair_events_batch, beside the `abi` table that
    tests/test_clj_shim.py holds to its exact set of structs -- equals the ctypes binding; every (po :struct :field) of the code names an
    entry of it; pair-events-batch invokes the exported symbol."""
    import re
    from test_clj_shim import SHIM, top_level_forms
    from jepsen_tigerbeetle_amd.jepsen import edn
    src = open(SHIM).read()
    forms = [src[a:b] for a, b in top_level_forms(src)]
    (f,) = [x for x in forms if x.startswith("(def pair-abi")]
    tab = edn.loads(f[len("(def pair-abi"):-1])
    structs = {"event_batch": N.EventBatch, "pair_out": N.PairOut}
    assert set(tab) == set(structs)
    for name, cls in structs.items():
        t = dict(tab[name])
        assert t.pop("size") == C.sizeof(cls), name
        assert set(t) == {x[0] for x in cls._fields_}, name
        for field, off in t.items():
            assert getattr(cls, field).offset == off, (name, field)
    code = re.sub(r";[^\n]*", "", "\n".join(x for x in forms if not x.startswith("(def pair-abi")))
    uses = re.findall(r"\(po\s+:([a-z_]+)\s+:([a-z_0-9]+)\)", code)
    assert len(uses) >= 20
    for s, k in uses:
        assert s in tab and k in tab[s], (s, k)
    assert re.search(r'\(defn pair-events-batch\b', src) and '(f "tbc_pair_events_batch")' in src
    assert hasattr(native.lib(), "tbc_pair_events_batch")

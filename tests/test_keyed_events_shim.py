"""clj/src/tigerbeetle/checker/gpu_linear.clj, one keyed history: `keyed-abi` -- the structs of tbc_pair_keyed_events and of tbc_batch_map_keyed_events /
tbc_batch_submit_keyed_events, in a table of
their own beside `abi`, `pair-abi` and `events-abi` -- equals the ctypes binding; every (ko :struct :field) of the code names an entry
of it; pair-keyed-events, map-keyed-events and submit-keyed-events invoke the exported symbols."""
import ctypes as C
import re

from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import edn
from test_clj_shim import SHIM, top_level_forms


def test_the_shim_binds_the_entry_point_by_its_own_table(native):
    src = open(SHIM).read()
    forms = [src[a:b] for a, b in top_level_forms(src)]
    (f,) = [x for x in forms if x.startswith("(def keyed-abi")]
    tab = edn.loads(f[len("(def keyed-abi"):-1])
    structs = {"keyed_events": N.KeyedEvents, "split_out": N.SplitOut, "batch_keyed_events": N.BatchKeyedEvents, "keyed_report": N.KeyedReport}
    assert set(tab) == set(structs)
    for name, cls in structs.items():
        t = dict(tab[name])
        assert t.pop("size") == C.sizeof(cls), name
        assert set(t) == {x[0] for x in cls._fields_}, name
        for field, off in t.items():
            assert getattr(cls, field).offset == off, (name, field)
    code = re.sub(r";[^\n]*", "", "\n".join(x for x in forms if not x.startswith("(def keyed-abi")))
    uses = re.findall(r"\(ko\s+:([a-z_]+)\s+:([a-z_0-9]+)\)", code)
    assert len(uses) >= 15 and {s for s, _ in uses} == set(structs)
    for s, k in uses:
        assert s in tab and k in tab[s], (s, k)
    # every field of either struct is set or read by the code
    assert {(s, k) for s, k in uses} >= {(s, k) for s in tab for k in tab[s] if k != "size" and not k.startswith("reserved")}
    for fn, symbol in (("pair-keyed-events", "tbc_pair_keyed_events"), ("map-keyed-events", "tbc_batch_map_keyed_events"),
                       ("submit-keyed-events", "tbc_batch_submit_keyed_events")):
        assert re.search(r"\(defn %s\b" % fn, src) and '(f "%s")' % symbol in src, fn
        assert hasattr(native.lib(), symbol)

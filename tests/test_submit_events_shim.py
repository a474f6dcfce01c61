"""clj/src/tigerbeetle/checker/gpu_linear.clj, events into a batch: `events-abi` -- the structs of tbc_batch_map_events and
tbc_batch_submit_events, in a table of their own beside `abi` and `pair-abi` -- equals the ctypes binding; every (eo :struct :field) of
the code names an entry of it; map-events / submit-events / pack-events invoke the exported symbols."""
import ctypes as C
import re

from jepsen_tigerbeetle_amd import _native as N
from jepsen_tigerbeetle_amd.jepsen import edn
from test_clj_shim import SHIM, top_level_forms


def test_the_shim_binds_the_entry_points_by_its_own_table(native):
    src = open(SHIM).read()
    forms = [src[a:b] for a, b in top_level_forms(src)]
    (f,) = [x for x in forms if x.startswith("(def events-abi")]
    tab = edn.loads(f[len("(def events-abi"):-1])
    structs = {"batch_events": N.BatchEvents, "events_report": N.EventsReport}
    assert set(tab) == set(structs)
    for name, cls in structs.items():
        t = dict(tab[name])
        assert t.pop("size") == C.sizeof(cls), name
        assert set(t) == {x[0] for x in cls._fields_}, name
        for field, off in t.items():
            assert getattr(cls, field).offset == off, (name, field)
    code = re.sub(r";[^\n]*", "", "\n".join(x for x in forms if not x.startswith("(def events-abi")))
    uses = re.findall(r"\(eo\s+:([a-z_]+)\s+:([a-z_0-9]+)\)", code)
    assert len(uses) >= 10 and {s for s, _ in uses} == set(structs)
    for s, k in uses:
        assert s in tab and k in tab[s], (s, k)
    for fn, symbol in (("pack-events", "tbc_pack_events"), ("map-events", "tbc_batch_map_events"), ("submit-events", "tbc_batch_submit_events")):
        assert re.search(r"\(defn %s\b" % fn, src) and '(f "%s")' % symbol in src, fn
        assert hasattr(native.lib(), symbol)

"""The keyed event histories tbc_pair_keyed_events is tested on, shared by the emulator test (tests/test_keyed_events_emu.py) and the
GPU test (tests/test_keyed_events_gpu.py): the smallest shapes at which each mechanism of csrc/split_kernels.h can go wrong -- chunks
of 64 rows and tiles of T = 1,024, the digits of the sort (n_keys around 2^8 and 2^16), the key table (sp::table_hash, stated below),
the order of the keys -- and the reference: columns.split_events in numpy, then tbc_pair_events key by key (pair_events_shapes.reference).
A case is a list of keyed histories (EventColumns, key int32[n]); each goes into one call.

THREE THRESHOLDS of the kernels lie above those shapes, and large_cases() / large_case() hold one history each side of none of
them but just past each: 2^20 rows (the scan's one workgroup over the block sums takes its SECOND step of 256 once thist has more
than 256 blocks of 1,024 words, n_tiles > 1,024; the row kernels' grid of 4,096 workgroups of 256 threads begins to stride), 8,192
tiles (8,388,608 rows: the tile kernels' grid begins to stride) -- and, at any size, THE TABLE'S END: a probe run that starts in
the last slots goes on in slot 0 (probe_run_wraps, a small case).  The large histories are built in numpy and go through the split
alone, once each; they are not in cases(), whose every entry the tests run three to nine times.  The scan's own block stride
(sp_sum_kernel / sp_apply_kernel above 4,096 blocks) would need 16.8 M rows and a 512 MB key table: left out on purpose, the
emulator's capped grids run that loop and the library's cap is one min."""
import functools

import numpy as np

import packed_events_shapes as PK
import pair_events_shapes as PS
from jepsen_tigerbeetle_amd import columns
from pair_events_shapes import FAIL, H, I, INFO, NIL, OK, R, W, pairs

T = 1024                      # sp::kTile: the rows one wavefront walks in the first-row count, the histogram and the scatter
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_M64 = (1 << 64) - 1


def table_bits(n):
    """sp::table_bits of csrc/split_plan.h: the table has 1 << bits slots, a power of two at or above 2n, 64 at least"""
    bits = 6
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


def table_hash(k, bits):
    """sp::table_hash of csrc/split_plan.h (the emulator test holds it against the C function): the top bits of a 64-bit product"""
    return (((k & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & _M64) >> (64 - bits)


def sort_passes(n_keys):
    """sp::sort_passes: the 8-bit passes of the sort on ids 0 .. n_keys - 1"""
    p, top = 0, max(n_keys - 1, 0)
    while top:
        p, top = p + 1, top >> 8
    return p


def interleave(evs, keys):
    """the histories `evs` (EventColumns), history i under key keys[i], as ONE history: round-robin, a row of each history that still
    has one in turn -> (EventColumns, key int32[n])"""
    lens = np.array([len(e) for e in evs], np.int64)
    hist = np.concatenate([np.full(m, i, np.int64) for i, m in enumerate(lens)]) if len(evs) else np.zeros(0, np.int64)
    pos = np.concatenate([np.arange(m) for m in lens]) if len(evs) else np.zeros(0, np.int64)
    order = np.lexsort((hist, pos))                      # by row within the history, then by history
    _, cat = columns.concat_events(evs)
    return columns.take_events(cat, order), np.asarray(keys, np.int64)[hist[order]].astype(np.int32)


def spread(n, n_keys, keys=None):
    """exactly n rows over n_keys keys, round-robin, every key's rows a well-formed history"""
    sizes = [n // n_keys + (1 if i < n % n_keys else 0) for i in range(n_keys)]
    return interleave([H(pairs(m, base=i)) for i, m in enumerate(sizes)], keys if keys is not None else [10 * i + 3 for i in range(n_keys)])


def colliding_keys(n, count):
    """`count` keys that hash to ONE slot of the table a history of n rows gets, and `count` more in the slot behind it (a probe run)"""
    bits = table_bits(n)
    h = table_hash(1, bits)
    same = [k for k in range(1, 200000) if table_hash(k, bits) == h][:count]
    behind = [k for k in range(1, 200000) if table_hash(k, bits) == (h + 1) % (1 << bits)][:count]
    assert len(same) == count and len(behind) == count
    return [int(k) for pair in zip(same, behind) for k in pair]


def wrapping_keys(n):
    """keys whose probe run crosses the END of the table a history of n rows gets: 8 whose home is the last slot, 8 in the slot before
    it, 4 in slot 0 -- a key of each in turn, so that the run that begins in slot 2^bits - 2 goes on through slots 0, 1, ... past the
    keys whose home slot 0 is"""
    bits = table_bits(n)
    last = (1 << bits) - 1
    at = lambda slot, count: [k for k in range(1, 200000) if table_hash(k, bits) == slot][:count]
    groups = [at(last, 8), at(last - 1, 8), at(0, 4)]
    assert [len(g) for g in groups] == [8, 8, 4]
    keys = [g[i] for i in range(8) for g in groups if i < len(g)]
    assert len(keys) == 20 and sum(table_hash(k, bits) == last for k in keys) >= 2
    return keys


def _cases():
    c = {}
    c["sizes"] = [spread(n, 3) for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)]
    c["one_key"] = [(H(pairs(2 * T + 1, procs=tuple(range(5)))), np.full(2 * T + 1, 5, np.int32))]
    n = T + 70
    c["every_row_its_own_key"] = [(H([(I, 1, W, r % 5, 0) for r in range(n)]), (np.arange(n)[::-1] * 7 - 3000).astype(np.int32))]
    # the digits of the sort: one 8-bit pass holds 256 keys, two hold 65,536
    rng = np.random.default_rng(7)
    c["digit_edges_8"] = [(H([(I, 0, W, r % 5, 0) for r in range(nk)]), rng.permutation(nk).astype(np.int32) - 100) for nk in (255, 256, 257)]
    c["digit_edges_16"] = [(H([(I, 0, W, r % 5, 0) for r in range(nk)]), (rng.permutation(nk) * 3 - 70000).astype(np.int32)) for nk in (65535, 65536, 65537)]
    c["two_keys_alternating"] = [spread(4 * T + 2, 2, keys=[9, -9])]
    # the keys' FIRST rows in descending key order (and their later rows in ascending order of the key)
    desc = list(range(1000, 1000 - 12, -1))
    ev, key = interleave([H(pairs(6, base=i)) for i in range(12)], desc)
    c["first_appearance_descending"] = [(ev, key), (H(pairs(8)), np.array([3, 2, 1, 1, 2, 3, 0, 0], np.int32))]
    c["key_values"] = [spread(200, 4, keys=[INT32_MAX, -1, INT32_MIN, 0]), spread(9, 4, keys=[-1, INT32_MIN, INT32_MAX, 0])]
    c["colliding_keys"] = [spread(300, 24, keys=colliding_keys(300, 12))]
    # a probe run across the table's end: the `& mask` step from the last slot to slot 0, in the insert and in the lookup
    c["probe_run_wraps"] = [spread(300, 20, keys=wrapping_keys(300))]
    # two passes of the sort with up to 16 rows a key, every key's rows in four or five tiles: the order of a key's OWN rows through a second
    # stable pass; key values scattered, not in the order of first appearance
    c["many_rows_over_passes"] = [spread(4 * T + 3, 257, keys=[(i * 7919) % 65521 - 30000 for i in range(257)])]
    # an invocation in the last row of a chunk / of a tile of the ONE history, its completion in the first row of the next -- and the same
    # at row 63 / 64 of the key's own rows (the pairing's chunk)
    rows, key = [], []
    filler = pairs(4 * T)
    fk = lambda r: 100 + (r // 2) % 3                    # (an invocation and its completion under one key; fillers use processes 0..2)
    special = {63: (I, 50, 7), 64: (OK, 50, 7), T - 1: (I, 51, 8), T: (OK, 51, 8), 2 * T + 63: (I, 52, 8), 2 * T + 64: (FAIL, 52, 8), 3 * T - 1: (I, 53, 7), 3 * T: (INFO, 53, 7)}
    k = 0
    for r in range(3 * T + 200):
        if r in special:
            ty, p, kk = special[r]
            rows.append((ty, p, W, 1, 0)); key.append(kk)
        else:
            rows.append(filler[k]); key.append(fk(k)); k += 1
    own = pairs(62) + [(I, 70, W, 2, 0), (I, 71, R, NIL, 0), (OK, 71, R, 4, 0), (OK, 70, W, 2, 0)]     # key 9's own rows 63 / 64
    ev9, key9 = interleave([H(own), H(pairs(300)), H(pairs(10))], [9, 4, 2])
    c["chunk_and_tile_edges"] = [(H(rows), np.array(key, np.int32)), (ev9, key9)]
    # refusal is per key: a malformed key and a key of 4,097 processes among good ones
    many = H([(I, p, W, p % 5, 0) for p in range(4097)] + [(OK, p, W, p % 5, 0) for p in range(4097)])
    bad = H(pairs(20) + [(OK, 9, W, 1, 0)] + pairs(6))
    c["refusal_per_key"] = [interleave([H(pairs(100)), bad, H(pairs(65)), many, H(pairs(129)), H([(5, 1, W, 0, 0)]), H(pairs(3))], [1, 2, 3, 4, 5, 6, 7])]
    # the semantics of tbc_pair_events and the wire format's limits, through the split
    sem, wire = PS.cases()["semantics"], PS.cases()["wire"]
    c["semantics"] = [interleave(sem, [50 - 3 * i for i in range(len(sem))])]
    c["wire"] = [interleave(wire, [7 * i - 20 for i in range(len(wire))])]
    return c


WORD_CASES = ("wire", "sizes", "semantics", "refusal_per_key")
BIG_CASES = ("digit_edges_16",)          # ~200k rows, a key each: the emulator test runs the SPLIT of these alone, at grids 3 and 1 with a seed each (a
                                         # wavefront of the pairing clears a 4,096-entry table per key: most of a minute on the CPU); the GPU test pairs them


# ---- the large shapes: past 2^20 rows and past 8,192 tiles
LARGE_CASES = ("top_scan_second_step", "top_scan_three_passes", "three_passes_many_rows")     # the emulator and the GPU
LARGE_GPU_CASES = LARGE_CASES + ("tiles_stride",)                                             # (8.4 M rows: the GPU alone)
_LARGE = {"top_scan_second_step": (T * T + 1, 300, 11), "top_scan_three_passes": (T * T + T + 1, 70000, 12),
          "three_passes_many_rows": (3 * 65537 + 5, 65537, 13), "tiles_stride": (8192 * T + T + 1, 1000, 14)}


def _large(n, n_keys, seed):
    """n rows over n_keys keys, in numpy: every key once in the order of its id (an invocation of process 0 that never completes),
    then invocation and :ok of a process 1..3 in ADJACENT rows under one key drawn at random, and an invocation of process 4 in the
    last row where rows are left over -- every key's rows a well-formed history.  The key VALUES are a seeded permutation, spread out:
    not in the order of first appearance."""
    rng = np.random.default_rng(seed)
    m = (n - n_keys) // 2
    drawn = rng.integers(0, n_keys, m)
    ids = np.concatenate([np.arange(n_keys), np.repeat(drawn, 2), rng.integers(0, n_keys, (n - n_keys) % 2)])
    k = np.arange(m)
    typ = np.concatenate([np.full(n_keys, I), np.tile([I, OK], m), np.full((n - n_keys) % 2, I)]).astype(np.uint8)
    proc = np.concatenate([np.zeros(n_keys, np.int64), np.repeat(1 + k % 3, 2), np.full((n - n_keys) % 2, 4)]).astype(np.int32)
    a = np.concatenate([np.arange(n_keys) % 5, np.repeat(k % 5, 2), np.zeros((n - n_keys) % 2, np.int64)]).astype(np.int32)
    value = (rng.permutation(n_keys) * 29 - 1000000).astype(np.int32)
    ev = columns.EventColumns(typ, proc, np.full(n, W, np.uint8), a, np.zeros(n, np.int32))
    assert len(ev) == len(ids) == n
    return ev, np.ascontiguousarray(value[ids])


@functools.lru_cache(maxsize=None)
def large_case(name):
    """(EventColumns, key int32[n]) of one large shape, built once; each holds in Python what it is named for"""
    n, n_keys, seed = _LARGE[name]
    ev, key = _large(n, n_keys, seed)
    n_tiles, per_key = (n + T - 1) // T, np.bincount(np.unique(key, return_inverse=True)[1].reshape(-1))
    blocks = (256 * n_tiles + 1023) // 1024                      # of the scan over thist
    assert len(per_key) == n_keys and per_key.min() >= 1 and per_key.max() >= 3
    if name == "top_scan_second_step":                           # 257 blocks: ONE into the second step; the row kernels stride
        # (block 256 is the last tiles of digit 255: the key of id 255 has rows there, so the step's carried base places rows)
        assert (n, n_tiles, blocks, sort_passes(n_keys)) == (T * T + 1, T + 1, 257, 2) and n > 4096 * 256
        assert (key[(n_tiles - 200) * T:] == key[255]).any() and not (key[:255] == key[255]).any()
    elif name == "top_scan_three_passes":                        # the same with a third pass: the final buffers are id_b / row_b
        assert n == T * T + T + 1 and blocks > 256 and sort_passes(n_keys) == 3 and len(set(key[:2 * 65537].tolist())) >= 65537
    elif name == "three_passes_many_rows":                       # a key's own rows through three stable passes
        assert (n, n_keys, sort_passes(n_keys)) == (3 * 65537 + 5, 65537, 3) and np.array_equal(np.unique(key[:n_keys]), np.unique(key))
    else:                                                        # tiles_stride: more tiles than the tile kernels' grid of 8,192
        assert n_tiles == 8194 > 8192 and blocks > 256 and sort_passes(n_keys) == 2
    return ev, key


def large_cases():
    """name -> (EventColumns, key) of the large shapes the emulator runs (tiles_stride: large_case, the GPU test alone)"""
    return {name: large_case(name) for name in LARGE_CASES}


@functools.lru_cache(maxsize=None)
def large_reference(name):
    """columns.split_events of a large shape, computed once and shared: keys, ev_off, row_of, n_keys"""
    ev, key = large_case(name)
    keys, ev_off, row_of = columns.split_events(ev, key)
    return {"keys": keys, "ev_off": ev_off, "row_of": row_of, "n_keys": len(keys)}


def forms(name):
    """(packed, word) of the calls a case goes through: the five columns, with the wire word where the case is about it; the packed form
    as a batch asks (the wire word)"""
    return [(False, False)] + ([(False, True)] if name in WORD_CASES else []) + [(True, True)]


_CASES = None
_REFS = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def _all_keys_fine(moved, off, word):
    """tbc_pair_events key by key over the split rows `moved`, WITHOUT a numpy array per key (65,537 keys take seconds otherwise): the
    reference of a history in which every key is well-formed, has 4,096 processes at most and -- with `word` -- fits the wire format;
    None otherwise, and pair_events_shapes.reference states the rest of the contract."""
    import ctypes as C
    from jepsen_tigerbeetle_amd import _native as N
    n, nh = len(moved), len(off) - 1
    m = max(n, 1)
    out = {"f": np.zeros(m, np.uint8), "a": np.zeros(m, np.int32), "b": np.zeros(m, np.int32), "process": np.zeros(m, np.int32),
           "inv_pos": np.zeros(m, np.uint32), "ret_pos": np.zeros(m, np.uint32)}
    size = {"f": 1, "a": 4, "b": 4, "process": 4, "inv_pos": 4, "ret_pos": 4}
    ct = {"f": C.c_uint8, "a": C.c_int32, "b": C.c_int32, "process": C.c_int32, "inv_pos": C.c_uint32, "ret_pos": C.c_uint32}
    at = lambda arr, first, width, t: C.cast(arr.ctypes.data + first * width, C.POINTER(t))
    fn = N.lib().tbc_pair_events
    op_off, n_process = np.zeros(nh + 1, np.uint64), np.zeros(nh, np.uint32)
    k, npr, e, total = C.c_uint32(0), C.c_uint32(0), N.Events(), 0
    for h in range(nh):
        lo, e.n = int(off[h]), int(off[h + 1] - off[h])
        e.type, e.process, e.f = at(moved.type, lo, 1, C.c_uint8), at(moved.process, lo, 4, C.c_int32), at(moved.f, lo, 1, C.c_uint8)
        e.a, e.b = at(moved.a, lo, 4, C.c_int32), at(moved.b, lo, 4, C.c_int32)
        if fn(C.byref(e), *[at(out[c], total, size[c], ct[c]) for c in ("f", "a", "b", "process", "inv_pos", "ret_pos")], C.byref(k), C.byref(npr)) != 0 or npr.value > PS.TABLE:
            return None
        total += k.value
        op_off[h + 1], n_process[h] = total, npr.value
    ref = {c: v[:total] for c, v in out.items()}
    if word:
        w = PS.wire_reference(columns.OpColumns(*[ref[c] for c in ("f", "a", "b", "process", "inv_pos", "ret_pos")], n_events=n, n_process=0)) if total else np.zeros(0, np.uint32)
        if w is None:
            return None
        ref["word"] = w
    ref.update(status=np.zeros(nh, np.int32), bad_row=np.full(nh, 0xFFFFFFFF, np.uint32), n_events=np.diff(off).astype(np.uint32), n_process=n_process,
               op_off=op_off, n_ops=total, n_bad=0)
    return ref


def reference(name, i, ev, key, word, packed=False):
    """what tbc_pair_keyed_events must give for history i of case `name`: split_events in numpy, then tbc_pair_events per key
    (computed once and kept).  packed: over the events the packed words DECODE to (packed_events_shapes.py: a value the wire format
    does not hold comes back as 256, an :f above 15 as 16, an unknown type as 7)."""
    ref = _REFS.get((name, i, word, packed))
    if ref is None:
        if packed:
            ev = PK.decode(PK.pack(ev), ev.process)
        keys, ev_off, row_of = columns.split_events(ev, key)
        moved, off = columns.take_events(ev, row_of), ev_off.astype(np.int64)
        ref = _all_keys_fine(moved, off, word)
        if ref is None:
            evs = [columns.EventColumns(*[getattr(moved, c)[off[h]:off[h + 1]] for c in ("type", "process", "f", "a", "b")]) for h in range(len(keys))]
            ref = dict(PS.reference(("keyed", name, i, packed), evs, word))
        ref.update(keys=keys, ev_off=ev_off, row_of=row_of, n_keys=len(keys))
        _REFS[(name, i, word, packed)] = ref
    return ref


def assert_same(got, want, what, row_of=True, paired=True):
    """the split bit for bit, then every array of the pairing (pair_events_shapes.assert_same)"""
    assert got["n_keys"] == want["n_keys"], (what, got["n_keys"], want["n_keys"])
    for k in ("keys", "ev_off") + (("row_of",) if row_of else ()):
        if not np.array_equal(got[k], want[k]):
            at = int(np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[0]) if len(got[k]) == len(want[k]) else -1
            raise AssertionError((what, k, "first difference at", at, got[k][at:at + 4], want[k][at:at + 4]))
    if paired:
        PS.assert_same(got, want, what)


def packed(ev):
    """the packed form of a history: (ev_word, process)"""
    return columns.pack_events(ev), ev.process

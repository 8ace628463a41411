"""Scratch memory of the host entry points: what a call takes from the context's buffer pool it gives back, on every exit.

Every entry point of libcfhip.so takes its device scratch through one guard (cf_scratch, cf_common.h).  Two checks on an Engine,
shared by test_emu_scratch.py (host emulator) and test_gpu_scratch.py (MI355X):

  check_balanced   the entry points that use scratch, on the smallest inputs the other checkers build, every result against that
                   checker's own reference; the whole sequence over and over on one engine, and stats()["hbm_bytes_live"] after
                   every call of one round equal to the value after the same call of the round before.  A buffer that an exit
                   forgets, or one released with another size than it was taken with, shows as a difference.  (The figure counts
                   what the context keeps between calls as well — the k-mer set, the resident sequences of cf_hpc — so the
                   round that starts on a fresh context is not one of the two compared: it sets the state both start from.)
  check_refusals   the calls that fail AFTER scratch was taken, by a decision of host code (no device fault): each one twice, the
                   figure after the second refusal equal to the one after the first, and a good sequence afterwards.

The inputs: shapecheck.repeats_case(1, 4, 0) and cloud_size_case(513) for A1 - A6 and the placement, and the first case of
mapcheck, scorecheck, editcheck and tandemcheck that gives the kernels work (editcheck's first pair is two empty strings,
tandemcheck's first case has no reads: neither reaches an allocation), and xchcheck's smallest record set for the device steps of
the table exchange (cf_selftest_owner_buckets, cf_selftest_merge_records) with their twins cf_reset_table + cf_merge_table and
cf_or_unique_mask, and one small call of each selftest export of cf_prims.hip.  sequence(engine, steps) runs a part of it: the emulator
test uses it to walk every exit that a failed allocation takes."""
import copy
import ctypes as C
import json
import os

import numpy as np

import editcheck
import mapcheck
import primcheck
import scorecheck
import shapecheck
import tandemcheck
import xchcheck
from centroflye_amd import session
from centroflye_amd.engine import DeviceError
from oracle import cport, placer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


class Traced:
    """An Engine whose every call leaves (method, hbm_bytes_live after it) in .log, whether it returned or raised."""

    def __init__(self, engine):
        self.engine, self.log = engine, []

    def __getattr__(self, name):
        f = getattr(self.engine, name)
        if not callable(f) or name in ("stats", "times", "set_param", "get_param", "knobs"):
            return f

        def call(*a, **kw):
            try:
                return f(*a, **kw)
            finally:
                self.log.append((name, self.engine.stats()["hbm_bytes_live"]))
        return call


def _inputs():
    """Built once and left unchanged (each case keeps the reference it was given by its own checker)."""
    if not _CACHE:
        _CACHE["repeats"] = shapecheck.repeats_case(1, 4, 0)
        _CACHE["cloud513"] = shapecheck.cloud_size_case(513)
        _CACHE["map_cases"] = mapcheck.load_cases()
        _CACHE["score_cases"] = scorecheck.load_cases()
        _CACHE["edit"] = next((a, b) for _, a, b in editcheck.single_cases(small_only=True) if a and b)
        _CACHE["hpc"] = editcheck.hpc_case(long_runs=False)
        _CACHE["tandem_golden"] = tandemcheck.load_cases()
        _CACHE["tandem"] = next(c for c in tandemcheck.cases() if c["reads"])
        with open(os.path.join(ROOT, "tests", "golden", "rr_vectors.json")) as f:
            _CACHE["rr"] = next(v for v in json.load(f) if len(v["unit"]) > 1)
        rng = np.random.default_rng(17)
        _CACHE["sort"] = rng.integers(0, 2 ** 40, 2 * shapecheck.TILE + 3, dtype=np.uint64)
        _CACHE["scan"] = rng.integers(0, 2 ** 36, 2 * 2048 + 5, dtype=np.int64)
        _CACHE["xch_records"] = min((c for c in xchcheck.merge_cases() if c["recs"]), key=lambda c: len(c["recs"]))
    return _CACHE


def _a1_a6(e, case):
    """load -> count -> select -> clouds -> dist -> filter by shapecheck.check_shapes (with set_kmers, clouds and dist on a thinned
    set where the literal loops of the reference would take too long), then the calls on the edges and the unique bitmap."""
    nv = shapecheck.check_shapes(e, case)
    ref = case.get("thin") or nv              # what the edges in memory were computed from
    n = ref["edges"].shape[0]
    e.sort_edges()
    got = e.edges(n).astype(np.int64)
    assert np.array_equal(got, ref["edges"]), case["name"] + ": sorted edges"
    assert e.edges_checksum(n) == cport.edge_checksum(got), case["name"] + ": edge checksum"
    mask = e.unique_mask()
    assert np.array_equal(np.flatnonzero(mask), ref["unique"])
    e.reset_unique()
    e.or_unique_mask(mask)
    assert np.array_equal(e.unique_mask(), mask) and e.stats()["n_unique"] == int(mask.sum())


def _place(e, case):
    """The greedy placement on the clouds that _a1_a6 left, both implementations, against the oracle's loop."""
    R = len(case["reads"])
    ids = [f"r{i}" for i in range(R)]
    cls = np.ones(R, np.uint8)
    cls[0] = 0
    unit_ptr = shapecheck.to_arrays(case["reads"], case["units"])[2]
    cp, ent = e.clouds()
    want = placer.place_reads(ids, cls.astype(np.int64), unit_ptr, cp, ent, 2, 2, 10, 3)
    for mode in (1, 2):
        with e.knobs(place_mode=mode):
            rd, pos, s0, s1 = e.place_reads(cls, np.arange(R, dtype=np.int32), 2, 2, 10, 3)
        got = [f"{ids[a]} 0" if (c < 0 and b == 0) else (f"{ids[a]} None" if b < 0 else f"{ids[a]} {b} {c} {d}")
               for a, b, c, d in zip(rd.tolist(), pos.tolist(), s0.tolist(), s1.tolist())]
        assert got == want, f"{case['name']}: placement, place_mode {mode}"


def _sources(e, report):
    """mapcheck.Sources on the traced engine: the fixture's clouds are installed through the package's session, which has to own
    the engine itself."""
    session.reset()
    session._engine = e.engine if isinstance(e, Traced) else e
    src = mapcheck.Sources(session._engine, report, _inputs()["map_cases"])
    return src


def _map_and_score(e, report, source=None):
    """contig_build, map_reads (first case of mapcheck), score_reads and contig_spread (first case of scorecheck); source: the
    first cases of that source of the goldens ("hand": a CSR of 14 reads that needs no fixture)."""
    inp = _inputs()
    src = _sources(e, report)
    try:
        m = next(c for c in inp["map_cases"]["cases"] if source in (None, c["source"]))
        s = next(c for c in inp["score_cases"]["cases"] if source in (None, c["source"]))
        src.use(m["source"])
        seen = copy.copy(src)
        seen.engine = e                          # (the clouds are installed: the calls of the cases go through the trace)
        mapcheck.check_case(seen, m)
        assert s["source"] == m["source"]
        scorecheck.check_case(seen, s)
        # every read asked for many times over: buffers of a size that no call before has left in the pool
        R = len(src.state[0])
        q = np.tile(np.arange(R, dtype=np.int64), -(-MANY_QUERIES // R))
        for ask in (lambda r: e.map_reads(r, m["threshold"]), lambda r: e.score_reads(r, 0, s["max_pos"], *s["threshold"])):
            once, many = ask(None), ask(q)
            assert all(np.array_equal(np.tile(a, q.size // R), b) for a, b in zip(once, many))
    finally:
        session._engine = None
        session.reset()


def _edit(e):
    inp = _inputs()
    data, off, seqs = inp["hpc"]
    out, out_off = e.hpc(data, off)
    want = [editcheck.hpc(s) for s in seqs]
    assert bytes(out) == b"".join(want) and np.diff(out_off).tolist() == [len(w) for w in want]
    # every sequence against its compressed form (deletions alone), on the bytes that hpc left on the device
    d, _ = e.edit_distances(None, off, out_off + int(off[-1]), 50)
    assert d.tolist() == [len(s) - len(w) if len(s) - len(w) <= 50 else -1 for s, w in zip(seqs, want)]
    a, b = inp["edit"]
    assert editcheck.one_pair(e, a, b) == editcheck.nw(a, b)


def _tandem(e):
    inp = _inputs()
    tandemcheck.check_case(e, inp["tandem_golden"], inp["tandem"])


def _rr(e):
    v = _inputs()["rr"]
    read = v["read"].encode()
    fwd, rc = e.rr_distances(v["unit"].encode(), np.frombuffer(read, np.uint8), [0, len(read)], v["threshold"])
    assert (int(fwd[0]), int(rc[0])) == (v["fwd"], v["rc"])


def _selftests(e):
    inp = _inputs()
    assert np.array_equal(e.selftest_sort(inp["sort"], 40), np.sort(inp["sort"]))
    assert np.array_equal(e.selftest_scan(inp["scan"]), np.concatenate([[0], np.cumsum(inp["scan"])]))
    # the other primitives of cf_prims.hip, each with scratch of its own and the primitive's (primcheck holds their cases)
    assert np.array_equal(e.selftest_scan_inplace(inp["scan"]), np.concatenate([[0], np.cumsum(inp["scan"])]))
    counts = (inp["scan"] & 0xFFFFFFFF).astype(np.uint32)
    assert np.array_equal(e.selftest_scan_u32(counts), primcheck.reference_scan(counts))
    recs = primcheck.records(counts.size, {1: counts})
    primcheck.check_sort(e, recs, [1], [24], "scratch")
    primcheck.check_offsets(e, counts[:17 * 65].reshape(17, 65) >> np.uint32(16), "scratch")

def _exchange(e):
    """The device steps of the table exchange for a virtual world and their host-mediated twins, on xchcheck's smallest records
    (codes 0 and 2^62 - 1, each twice), every result as xchcheck checks it."""
    case = _inputs()["xch_records"]
    xchcheck.check_merge(e, case)
    table = {x: list(v) for x, v in xchcheck.expected_merge(case["recs"]).items()}
    xchcheck.check_buckets(e, table, 3, "scratch: " + case["name"])
    xchcheck.check_merge(e, case, parts=1)
    xchcheck.check_or_unique_mask(e, xchcheck.MASK_SIZES[2])


STEPS = ("a1_a6", "place", "cloud513", "map_score", "edit", "tandem", "rr", "selftests", "exchange")
MANY_QUERIES = 700
SMALL_STEPS = ("a1_a6", "map_score_hand", "tandem", "exchange")      # a sequence of a tenth of a second on the emulator


def sequence(e, report, steps=STEPS):
    """The named parts in order on e (an Engine or a Traced one); a DeviceError of any call ends it."""
    inp = _inputs()
    for step in steps:
        if step == "a1_a6":
            _a1_a6(e, inp["repeats"])
        elif step == "place":
            _place(e, inp["repeats"])
        elif step == "cloud513":
            _a1_a6(e, inp["cloud513"])
            _place(e, inp["cloud513"])
        elif step == "map_score":
            _map_and_score(e, report)
        elif step == "map_score_hand":
            _map_and_score(e, report, "hand")
        elif step == "edit":
            _edit(e)
        elif step == "tandem":
            _tandem(e)
        elif step == "rr":
            _rr(e)
        elif step == "selftests":
            _selftests(e)
        elif step == "exchange":
            _exchange(e)
        else:
            raise ValueError(step)


def check_balanced(engine, report, steps=STEPS):
    sequence(engine, report, steps)
    rounds = []
    for _ in range(2):
        t = Traced(engine)
        sequence(t, report, steps)
        rounds.append(t.log)
    assert [n for n, _ in rounds[0]] == [n for n, _ in rounds[1]] and len(rounds[0]) > 20
    bad = [(i, a[0], a[1], b[1]) for i, (a, b) in enumerate(zip(*rounds)) if a[1] != b[1]]
    assert not bad, f"hbm_bytes_live differs between two rounds of the same calls: first (call, method, round 1, round 2) {bad[:3]}"
    return rounds[0]


def _refused(engine, code, what, call):
    live = []
    for _ in range(2):
        try:
            call()
        except DeviceError as err:
            assert f"({code})" in str(err) and what in str(err), str(err)
        else:
            raise AssertionError(f"the call was not refused ({what})")
        live.append(engine.stats()["hbm_bytes_live"])
    assert live[0] == live[1], f"{what}: hbm_bytes_live {live[0]} after the first refusal, {live[1]} after the second"


def check_refusals(engine, report):
    inp = _inputs()
    # a unit with more set k-mers than the LDS cloud set holds: both attempts of cf_build_clouds have run by then
    big = _CACHE.setdefault("cloud6145", shapecheck.cloud_size_case(6145))
    live = []
    for _ in range(2):
        shapecheck.check_shapes(engine, big)       # (asserts the -34 itself)
        live.append(engine.stats()["hbm_bytes_live"])
    assert live[0] == live[1], f"refused cloud: hbm_bytes_live {live}"
    # an unsorted k-mer set: found by the kernel that builds the lookup table, after the set and its tables are allocated
    _refused(engine, -22, "sorted", lambda: engine.set_kmers(np.array([5, 3, 9], np.uint64), 4))
    # 1025 keys into the 1024 slots of cf_reset_table(k, 0): found by the merge kernel, after the records and the flags are allocated
    full = (np.arange(1, 1026, dtype=np.uint64), np.ones(1025, np.uint32), np.zeros(1025, np.uint32))
    _refused(engine, -34, "table full", lambda: (engine.reset_table(31, 0), engine.merge_table(*full)))
    # cf_contig_spread with room for one rank less than there are: found after the flags and their scan
    src = _sources(engine, report)
    try:
        m = inp["map_cases"]["cases"][0]
        mapcheck.check_case(src, m)
        n = engine.contig_spread(0).size
        assert n > 1
        ranks, n_out = np.zeros(n, np.int32), C.c_int64()
        _refused(engine, -22, "do not fit", lambda: engine._check(
            engine._lib.cf_contig_spread(engine._ctx, 0, ranks.ctypes.data, n - 1, C.byref(n_out)), "cf_contig_spread"))
    finally:
        session._engine = None
        session.reset()
    check_balanced(engine, report)

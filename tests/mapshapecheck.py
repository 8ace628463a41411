"""cf_contig_build / cf_map_reads (cf_map.hip) on hand-built clouds at the kernels' shape borders: the builders and the bodies that
tests/test_emu_map_shapes.py runs on the host emulator and tests/test_gpu_map_shapes.py on an MI355X.

A case is a CSR written by hand (mapcheck.install_synthetic: one base per unit, ranks 0 .. K - 1): usually one long backbone read of
mostly empty clouds that carries chosen ranks at chosen positions, and a handful of small query reads.  The expected values are the
numpy statements mapcheck.contig / map_read and scorecheck.contig / score_read / spread, which the committed goldens pin to the
reference's CloudContig and which share no code with the kernels; where the construction fixes an answer the literal is asserted
too.  Every case carries `regime` checks that are evaluated on the numpy result alone, BEFORE the device is asked: the hit span,
the starts that hold a tie, P, max_pos, the key widths, the run lengths.  A case that drifted out of its branch fails there.
Besides the mapper's answers every case compares what the scorer reads from the same contig (score_reads over the full range,
contig_spread, n_exact_pairs, contig_info, the whole coverage), so both CSRs that the builder writes are observed.

scratchcheck's comparison of 700 tiled queries is the kernel against itself (one pass of cf_map_kernel against another); family 4
here (check_past_the_launch_cap) is the comparison against the rule: every one of 192 x n_cu + 5 answers against mapcheck.
All comparisons are integer-exact."""
import numpy as np

import mapcheck
import scorecheck
from mapcheck import DEFAULT_WINDOW, _ranges

MAX_WINDOW = 4096                     # the largest map_window accepted: 12 bytes of LDS per slot, 48 KB
WINDOWS = (64, 0, MAX_WINDOW)         # forced, the default (DEFAULT_WINDOW slots), forced
SPANS = ("W-1", "W", "W+1", "2W", "2W+1")
WINDOWS_OF_SPAN = {"W-1": 1, "W": 1, "W+1": 2, "2W": 2, "2W+1": 3}
UNIT_ENTRIES = (1, 63, 64, 65, 129)   # entries of one unit: 1, 1, 1, 2 and 3 strides of a wave's 64 lanes
ROW_POSITIONS = (1, 2, 500, 777)      # positions in the row of one rank
RUN_F = (1, 2, 3, 64, 65, 300)
RECORD_COUNTS = (4095, 4096, 4097)    # one tile of the radix sort (RX_TILE 4096)
SPREAD = (0, 1, 5)
# (b, c): max_pos in {2^b - 1, 2^b} and K in {2^c, 2^c + 1}.  Bits that hold 0 .. x: x.bit_length(), at least 1; the record is
# [rank | position], so the sort width is bits(max_pos) + bits(K - 1): b + c, b + c + 1, b + c + 1 and b + c + 2 for the four
# combinations: 8, 9, 9, 10 / 16, 17, 17, 18 / 24, 25, 25, 26 bits: either side of one, two and three 8-bit radix passes.
KEY_WIDTHS = ((4, 4), (8, 8), (21, 3))


def bits_that_hold(x):
    """Bits that hold 0 .. x (at least 1): the documented meaning, not the library's loop."""
    return max(1, int(x).bit_length())


# ------------------------------------------------------------------ a hand-built case
class Case:
    def __init__(self, name, K, f=1, thresholds=((1, 1),), spread=SPREAD):
        self.name, self.K, self.f, self.thresholds, self.spread = name, int(K), int(f), [tuple(t) for t in thresholds], tuple(spread)
        self.sizes, self.chunks, self.unit_ptr = [], [], [0]      # entries per unit, the entries, units per read
        self.backbone, self.queries, self.q_name = [], [], {}
        self.literal = {}         # (query name, index of the threshold) -> (pos, s0, s1) that the construction fixes
        self.regimes = []         # callables (ref, W): assertions on the numpy result alone
        self.figures = {}         # literals of the contig that the construction fixes: P, max_pos, n_freq_kmers, n_pairs, n_exact_pairs
        self._next_rank = 0
        self._ref = None

    def rank(self, n=1):
        """n ranks that nothing else of the case uses."""
        first = self._next_rank
        self._next_rank += n
        assert self._next_rank <= self.K, f"{self.name}: more ranks than K"
        return first if n == 1 else list(range(first, first + n))

    def read(self, units, at=None, query=None, literal=None):
        """A read of the given clouds (one list of ranks per unit); at: laid on the backbone there; query: asked for, under that name."""
        for u in units:
            u = np.unique(np.asarray(u, np.int64))
            assert u.size == len(u) and (u.size == 0 or (0 <= u[0] and u[-1] < self.K))
            self.sizes.append(u.size)
            self.chunks.append(u)
        self.unit_ptr.append(len(self.sizes))
        r = len(self.unit_ptr) - 2
        if at is not None:
            self.backbone.append((r, int(at)))
        if query is not None:
            self.q_name[query] = len(self.queries)
            self.queries.append(r)
            for t, triple in (literal or {}).items():
                self.literal[(query, t)] = tuple(triple)
        return r

    def bulk(self, sizes, entries, at):
        """One-unit backbone reads in bulk: sizes[j] entries of read j, laid at at[j]."""
        first = len(self.unit_ptr) - 1
        self.sizes.extend(int(s) for s in sizes)
        self.chunks.append(np.asarray(entries, np.int64))
        self.unit_ptr.extend(range(self.unit_ptr[-1] + 1, self.unit_ptr[-1] + 1 + len(sizes)))
        self.backbone.extend((first + j, int(p)) for j, p in enumerate(at))
        return first

    def ask(self, r, name):
        self.q_name[name] = len(self.queries)
        self.queries.append(r)

    @staticmethod
    def sparse(n, content):
        """n clouds, empty except where content says {position: ranks}."""
        assert all(0 <= p < n for p in content)
        return [content.get(p, []) for p in range(n)]

    def spec(self):
        cloud_ptr = np.concatenate([[0], np.cumsum(np.asarray(self.sizes, np.int64))])
        entries = np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.int64)
        assert entries.size == cloud_ptr[-1]
        return dict(unit_ptr=np.asarray(self.unit_ptr, np.int64), cloud_ptr=cloud_ptr, entries=entries.astype(np.int32), K=self.K)

    def reference(self):
        """The numpy statements' answers, computed once per case and left unchanged."""
        if self._ref is None:
            spec = self.spec()
            A = tuple(np.asarray(spec[k], np.int64) for k in ("unit_ptr", "cloud_ptr", "entries"))
            b_reads = np.array([r for r, _ in self.backbone], np.int64)
            b_pos = np.array([p for _, p in self.backbone], np.int64)
            c = mapcheck.contig(*A, b_reads, b_pos, self.f)
            sc = scorecheck.contig(*A, b_reads, b_pos, self.f)
            self._ref = dict(
                spec=spec, A=A, b_reads=b_reads, b_pos=b_pos, c=c, sc=sc,
                want=[mapcheck.map_all(*A, c, self.queries, t0, t1) for t0, t1 in self.thresholds],
                score=[[scorecheck.score_read(*A, sc, r, 0, None, t0, t1) for r in self.queries] for t0, t1 in self.thresholds],
                span=[mapcheck.hit_span(*A, c, r) for r in self.queries],
                spread={m: scorecheck.spread(sc, m) for m in self.spread})
        return self._ref

    # what the regime checks read
    def q(self, name):
        return self.q_name[name]

    def units_of(self, name):
        r = self.queries[self.q(name)]
        return self.unit_ptr[r + 1] - self.unit_ptr[r]

    def table(self, name, admissible=True):
        ref = self.reference()
        return start_table(ref["A"], ref["c"], self.queries[self.q(name)], admissible)

    def holders(self, name, score, admissible=True):
        """The starts of a query that score exactly (s0, s1)."""
        starts, s0, s1 = self.table(name, admissible)
        return starts[(s0 == score[0]) & (s1 == score[1])].tolist()


def start_table(A, c, r, admissible=True):
    """(starts, s0, s1) of read r over every start >= 0 that has a hit (admissible: and s + n <= P).  Read by the regime checks only;
    the expected answers are mapcheck.map_read's."""
    unit_ptr, cloud_ptr, entries = A
    u0, u1 = int(unit_ptr[r]), int(unit_ptr[r + 1])
    ent, unit = _ranges(cloud_ptr[u0:u1], cloud_ptr[u0 + 1:u1 + 1])
    x = entries[ent]
    seeds, owner = _ranges(np.searchsorted(c["seed_rank"], x, "left"), np.searchsorted(c["seed_rank"], x, "right"))
    i = unit[owner]
    s = c["seed_pos"][seeds] - i
    ok = s >= 0
    if admissible:
        ok &= s <= c["P"] - (u1 - u0)
    s, i = s[ok], i[ok]
    starts, s1 = np.unique(s, return_counts=True)
    s0 = np.bincount(np.searchsorted(starts, np.unique((s << 32) | i) >> 32), minlength=starts.size)
    return starts, s0, s1


def _triples(pos, s0, s1):
    return list(zip(pos.tolist(), s0.tolist(), s1.tolist()))


def check(engine, case, window=0, reverse=False):
    """The regime of the case from numpy alone, the literals of the construction against numpy, then the device against numpy."""
    ref = case.reference()
    W = window or DEFAULT_WINDOW
    tag = f"{case.name} (window {window})"
    c, sc = ref["c"], ref["sc"]
    assert case.regimes, f"{tag}: a case without a regime check"
    for regime in case.regimes:
        regime(ref, W)
    for (name, t), triple in case.literal.items():
        assert ref["want"][t][case.q(name)] == triple, f"{tag}: numpy gives {ref['want'][t][case.q(name)]} for {name}, the construction {triple}"
    numpy_figures = dict(P=c["P"], max_pos=c["max_pos"], n_freq_kmers=c["n_freq_kmers"], n_pairs=c["n_pairs"], n_exact_pairs=sc["n_exact_pairs"])
    for k, v in case.figures.items():
        assert numpy_figures[k] == v, f"{tag}: numpy gives {k} = {numpy_figures[k]}, the construction {v}"
    assert (sc["P"], sc["max_pos"]) == (c["P"], c["max_pos"]) and sc["all_rank"].size == c["n_pairs"]
    # ---- the device
    mapcheck.install_synthetic(engine, ref["spec"])
    q = np.asarray(case.queries, np.int64)
    with engine.knobs(map_window=window):
        for order in ((1, -1) if reverse else (1,)):
            what = tag + (" (backbone reversed)" if order < 0 else "")
            engine.contig_build(ref["b_reads"][::order], ref["b_pos"][::order], case.f)
            info = engine.contig_info()
            got = (info["n_positions"], info["max_pos"], info["n_freq_kmers"], info["n_pairs"], engine.contig_exact_info()["n_exact_pairs"])
            assert got == (c["P"], c["max_pos"], c["n_freq_kmers"], c["n_pairs"], sc["n_exact_pairs"]), f"{what}: contig figures {got}"
            assert np.array_equal(engine.contig_coverage(), c["coverage"]), f"{what}: coverage"
            for m, ranks in ref["spread"].items():
                assert np.array_equal(engine.contig_spread(m), ranks), f"{what}: spread k-mers, max_npos {m}"
            for t, (t0, t1) in enumerate(case.thresholds):
                got = _triples(*engine.map_reads(q, (t0, t1)))
                bad = [(n, g, w) for n, g, w in zip(case.q_name, got, ref["want"][t]) if g != w]
                assert not bad, f"{what}: map_reads under {(t0, t1)}: {len(bad)} of {len(got)} differ (name, device, numpy), first {bad[:3]}"
                got = _triples(*engine.score_reads(q, None, None, t0, t1))
                bad = [(n, g, w) for n, g, w in zip(case.q_name, got, ref["score"][t]) if g != w]
                assert not bad, f"{what}: score_reads under {(t0, t1)}: {len(bad)} of {len(got)} differ (name, device, numpy), first {bad[:3]}"
    return ref


# ------------------------------------------------------------------ family 1: window borders
def window_case(window, span_name):
    """One backbone read of L units at 0, the hits of every query between start a and start a + span - 1.
    ends        one unit whose rank sits at a and at a + span - 1 only: the windows in between are empty
    slot_last   (2, 2) in slot W - 1 of the first window, single hits at both ends of the span
    slot_first  (2, 2) in slot 0 of the second window, single hits at both ends
    tie         (2, 2) at a and at a + span - 1: in different windows from W + 1 on, the larger start wins
    lane        (2, 2) in slots 3 and 67 of the first window (one lane reduces both), single hits at both ends
    full        a read of exactly P units that scores (2, 2) at 0 and would score (2, 2) at 1
    over        the same with P + 1 units
    local_j, weak_j, ends2   (for family 4) one-window reads that map, one-window reads below (2, 2), a second two-ended read."""
    W = window or DEFAULT_WINDOW
    span = {"W-1": W - 1, "W": W, "W+1": W + 1, "2W": 2 * W, "2W+1": 2 * W + 1}[span_name]
    a = 5
    L = a + span + 6
    case = Case(f"window_{window}_{span_name}", K=64, f=1, thresholds=((1, 1), (2, 2)))
    at = {}

    def put(rank, *positions):
        for p in positions:
            at.setdefault(p, []).append(rank)
        return rank
    end = a + span - 1
    queries = []
    x = put(case.rank(), a, end)
    queries.append(("ends", [[x]], {0: (end, 1, 1), 1: (-1, 0, 0)}))
    if span >= W:
        z, y0, y1 = put(case.rank(), a, end), put(case.rank(), a + W - 1), put(case.rank(), a + W)
        lit = (a + W - 1, 2, 3 if span == W else 2)
        queries.append(("slot_last", [[y0, z], [y1]], {0: lit, 1: lit}))
    if span >= W + 1:
        z, y0, y1 = put(case.rank(), a, end), put(case.rank(), a + W), put(case.rank(), a + W + 1)
        lit = (a + W, 2, 3 if span == W + 1 else 2)
        queries.append(("slot_first", [[y0, z], [y1]], {0: lit, 1: lit}))
    t0, t1 = put(case.rank(), a, end), put(case.rank(), a + 1, end + 1)
    queries.append(("tie", [[t0], [t1]], {0: (end, 2, 2), 1: (end, 2, 2)}))
    if W >= 128:
        z, v0, v1 = put(case.rank(), a, end), put(case.rank(), a + 3, a + 67), put(case.rank(), a + 4, a + 68)
        queries.append(("lane", [[v0, z], [v1]], {0: (a + 67, 2, 2), 1: (a + 67, 2, 2)}))
    g0, g1 = put(case.rank(), 0, 1), put(case.rank(), 1, 2)
    queries.append(("full", Case.sparse(L, {0: [g0], 1: [g1]}), {0: (0, 2, 2), 1: (0, 2, 2)}))
    queries.append(("over", Case.sparse(L + 1, {0: [g0], 1: [g1]}), {0: (-1, 0, 0), 1: (-1, 0, 0)}))
    for j in range(6):
        l0, l1 = put(case.rank(), a + 10 + 3 * j), put(case.rank(), a + 11 + 3 * j)
        queries.append((f"local_{j}", [[l0], [l1]], {0: (a + 10 + 3 * j, 2, 2), 1: (a + 10 + 3 * j, 2, 2)}))
    for j in range(3):
        w = put(case.rank(), a + 20 + j)
        queries.append((f"weak_{j}", [[w]], {0: (a + 20 + j, 1, 1), 1: (-1, 0, 0)}))
    x2 = put(case.rank(), a + 1, end - 1)
    queries.append(("ends2", [[x2]], {0: (end - 1, 1, 1), 1: (-1, 0, 0)}))
    case.read(Case.sparse(L, at), at=0)
    for name, units, literal in queries:
        case.read(units, query=name, literal=literal)
    case.figures = dict(P=L, max_pos=L - 1)

    def regime(ref, Wrun):
        assert ref["c"]["P"] == L and ref["c"]["max_pos"] == L - 1
        assert case.units_of("full") == ref["c"]["P"] and case.units_of("over") == ref["c"]["P"] + 1
        assert case.holders("full", (2, 2)) == [0] and case.holders("full", (2, 2), admissible=False) == [0, 1]
        assert case.table("ends")[0].tolist() == [a, end], "the only hits are at a and a + span - 1"
        for name in ("ends", "tie", "slot_last", "slot_first", "lane"):
            if name in case.q_name:
                assert ref["span"][case.q(name)] == span and case.table(name)[0][0] == a, name
        assert case.holders("tie", (2, 2)) == [a, end] and max(case.table("tie")[1]) == 2
        if Wrun != W:      # (the smallest span is also run with one start per window)
            assert (Wrun, span) == (1, 63)
            return
        assert -(-span // W) == WINDOWS_OF_SPAN[span_name]
        if span > W:
            assert (end - a) // W >= 1, "the tied starts lie in different windows"
        if "slot_last" in case.q_name:
            pos = ref["want"][0][case.q("slot_last")][0]
            assert ((pos - a) // W, (pos - a) % W) == (0, W - 1), "the winner sits in the last slot of the first window"
        if "slot_first" in case.q_name:
            pos = ref["want"][0][case.q("slot_first")][0]
            assert ((pos - a) // W, (pos - a) % W) == (1, 0), "the winner sits in the first slot of the second window"
        if "lane" in case.q_name:
            h = case.holders("lane", (2, 2))
            assert [(s - a) // W for s in h] == [0, 0] and [(s - a) % 64 for s in h] == [3, 3] and h[1] - h[0] == 64
    case.regimes.append(regime)
    return case


_WINDOW_CASES = {}


def window_cases(window, span_name):
    if (window, span_name) not in _WINDOW_CASES:
        _WINDOW_CASES[(window, span_name)] = window_case(window, span_name)
    return _WINDOW_CASES[(window, span_name)]


def check_window_border(engine, window, span_name):
    case = window_cases(window, span_name)
    check(engine, case, window)
    if window == 64 and span_name == "W-1":      # the smallest span, one start per window: 63 windows
        check(engine, case, 1)


# ------------------------------------------------------------------ family 2: the admissible range
def last_start_case():
    """map_window 64.  Query `edge` (3 units): single hits at last - 63 and at last, so the span is exactly one window; start last + 1
    scores (2, 2) and is not admissible: it must not win, and admitted into the span it would add a second window.
    Query `zero` (3 units): (2, 2) at start 0 from q == i, and (2, 3) at start -1 from q == i - 1."""
    W, L = 64, 100
    case = Case("last_start", K=32, f=1, thresholds=((1, 1),))
    last = L - 3
    e0, e1, e2 = case.rank(3)
    z0, z1, z1b, z2a, z2b = case.rank(5)
    at = {last - 63: [e0], last: [e0], last + 1: [e1], last + 2: [e2], 0: [z0, z1b], 1: [z1, z2a, z2b]}
    case.read(Case.sparse(L, at), at=0)
    # unit 0 holds e0 (starts last - 63, last) and e1 (start last + 1); unit 1 holds e2 (start last + 1)
    case.read([[e0, e1], [e2], []], query="edge", literal={0: (last, 1, 1)})
    # unit 0: z0 at 0 -> start 0; unit 1: z1 at 1 -> start 0, z1b at 0 -> start -1; unit 2: z2a, z2b at 1 -> start -1
    case.read([[z0], [z1, z1b], [z2a, z2b]], query="zero", literal={0: (0, 2, 2)})
    case.figures = dict(P=L, max_pos=L - 1)

    def regime(ref, Wrun):
        assert Wrun == W and ref["c"]["P"] == L and case.units_of("edge") == 3
        assert case.table("edge")[0].tolist() == [last - 63, last] and ref["span"][case.q("edge")] == W, "exactly one window"
        starts, s0, s1 = case.table("edge", admissible=False)
        assert (starts.tolist(), s0.tolist(), s1.tolist()) == ([last - 63, last, last + 1], [1, 1, 2], [1, 1, 2]), "last + 1 would win"
        assert case.table("zero", admissible=False)[0].tolist() == [0], "no other start >= 0 has a hit"
    case.regimes.append(regime)
    return case, W


def gap_case(long):
    """Two backbone reads with a gap between them: P < max_pos + 1.  Query `far` (n units) scores best where the second backbone
    read ends, at start max_pos + 1 - n, which lies in (P - n, max_pos + 1 - n]; its admissible single hit wins.  Query `near`
    maps inside the second backbone read, beyond the gap, at a start that is still admissible (short: exactly at P - n).
    long: the contig is longer than the default window and `far` has admissible hits more than a window apart."""
    L1, g, L2 = (2300, 100, 400) if long else (10, 5, 10)
    n = 4
    case = Case(f"gap_{'long' if long else 'short'}", K=32, f=1, thresholds=((1, 1),))
    P, max_pos = L1 + L2, L1 + g + L2 - 1
    s_far = max_pos + 1 - n
    f0, f1, f2, f3 = case.rank(4)
    w_lo, w_hi = case.rank(2)
    n0, n1 = case.rank(2)
    s_near = L1 + g + 3                       # admissible: s_near <= P - 2
    weak = 2 if not long else 2 + DEFAULT_WINDOW + 50
    case.read(Case.sparse(L1, {1: [w_lo], weak: [w_hi]}), at=0)
    case.read(Case.sparse(L2, {L2 - 4: [f0], L2 - 3: [f1], L2 - 2: [f2], L2 - 1: [f3], 3: [n0], 4: [n1]}), at=L1 + g)
    case.read([[f0, w_lo, w_hi], [f1], [f2], [f3]], query="far", literal={0: (weak, 1, 1)})
    case.read([[n0], [n1]], query="near", literal={0: (s_near, 2, 2)})
    case.figures = dict(P=P, max_pos=max_pos)

    def regime(ref, Wrun):
        c = ref["c"]
        assert (c["P"], c["max_pos"]) == (P, max_pos) and c["P"] < c["max_pos"] + 1
        assert int((c["coverage"] == 0).sum()) == g and c["coverage"][L1:L1 + g].sum() == 0
        starts, s0, s1 = case.table("far", admissible=False)
        best = int(starts[np.lexsort((starts, s1, s0))[-1]])
        assert best == s_far and c["P"] - n < best <= c["max_pos"] + 1 - n, "the best start lies between P - n and max_pos + 1 - n"
        assert case.table("far")[0].tolist() == [1, weak]
        assert L1 + g <= s_near <= c["P"] - 2, "beyond the gap and admissible"
        if long:
            assert c["max_pos"] + 1 > DEFAULT_WINDOW and ref["span"][case.q("far")] > Wrun == DEFAULT_WINDOW
        else:
            assert s_near == c["P"] - 2, "exactly the last admissible start"
    case.regimes.append(regime)
    return case


def threshold_case():
    """One query with (3, 7) at start 10 and (2, 9) at start 20, under thresholds at, above and below both."""
    L = 40
    thresholds = ((3, 7), (4, 7), (3, 8), (2, 8), (2, 9), (2, 10), (1, 1), (0, 0), (-5, -5), (4, 0))
    answers = ((10, 3, 7), (-1, 0, 0), (-1, 0, 0), (20, 2, 9), (20, 2, 9), (-1, 0, 0), (10, 3, 7), (10, 3, 7), (10, 3, 7), (-1, 0, 0))
    case = Case("thresholds", K=64, f=1, thresholds=thresholds)
    a_ranks = [case.rank(3), case.rank(2), case.rank(2)]            # 3 units, 7 hits at start 10
    b_ranks = [case.rank(5), case.rank(4)]                          # 2 units, 9 hits at start 20
    miss = case.rank()                                              # a rank of the read that the contig does not hold
    at = {}
    for i, ranks in enumerate(a_ranks):
        at.setdefault(10 + i, []).extend(ranks)
    for i, ranks in enumerate(b_ranks):
        at.setdefault(20 + i, []).extend(ranks)
    case.read(Case.sparse(L, at), at=0)
    case.read([a_ranks[0] + b_ranks[0], a_ranks[1] + b_ranks[1], a_ranks[2]], query="two", literal=dict(enumerate(answers)))
    case.read([[miss]], query="miss", literal={t: (-1, 0, 0) for t in range(len(thresholds))})      # no hit: no start, whatever the thresholds
    case.figures = dict(P=L, max_pos=L - 1)

    def regime(ref, Wrun):
        starts, s0, s1 = case.table("two")
        assert (starts.tolist(), s0.tolist(), s1.tolist()) == ([10, 20], [3, 2], [7, 9]), "larger s1 with smaller s0 at the larger start"
        assert case.table("miss")[0].size == 0
    case.regimes.append(regime)
    return case


# ------------------------------------------------------------------ family 3: lane strides and rows
def unit_entries_case(n_e):
    """Units of n_e entries whose hits all fall on one start.  one: (5, 1, n_e); two: units on the neighbouring starts 5 and 6, the
    larger wins the tie; three: three units on start 5, s0 = 3 (units, not entries)."""
    case = Case(f"unit_entries_{n_e}", K=6 * n_e, f=1, thresholds=((1, 1),))
    one = case.rank(n_e) if n_e > 1 else [case.rank()]
    two = [case.rank(n_e) if n_e > 1 else [case.rank()] for _ in range(2)]
    three = [case.rank(n_e) if n_e > 1 else [case.rank()] for _ in range(3)]
    at = {5: one + two[0] + three[0], 6: three[1], 7: two[1] + three[2]}
    case.read(Case.sparse(12, at), at=0)
    case.read([one], query="one", literal={0: (5, 1, n_e)})
    case.read([two[0], two[1]], query="two", literal={0: (6, 1, n_e)})
    case.read(three, query="three", literal={0: (5, 3, 3 * n_e)})
    case.figures = dict(P=12, max_pos=11, n_freq_kmers=6 * n_e, n_pairs=6 * n_e, n_exact_pairs=6 * n_e)

    def regime(ref, Wrun):
        assert int(np.diff(ref["spec"]["cloud_ptr"]).max()) == 3 * n_e and -(-n_e // 64) == {1: 1, 63: 1, 64: 1, 65: 2, 129: 3}[n_e]
        assert [a.tolist() for a in case.table("one")] == [[5], [1], [n_e]]
        assert [a.tolist() for a in case.table("two")] == [[5, 6], [1, 1], [n_e, n_e]]
        assert [a.tolist() for a in case.table("three")] == [[5], [3], [3 * n_e]]
    case.regimes.append(regime)
    return case


def row_case(npos):
    """Rank X at the positions 3 .. 3 + npos - 1: a row of npos positions.  The query [[X], [X]] scores (2, 2) at every start from 3
    to npos + 1 and (1, 1) at npos + 2 (and at 2): the largest start with (2, 2) wins, or (1, 1) at 3 for a row of one."""
    L = npos + 10
    case = Case(f"row_{npos}", K=4, f=1, thresholds=((1, 1),), spread=(0, 1, 5, npos - 1, npos))
    x, y = case.rank(2)
    at = {3 + p: [x] for p in range(npos)}
    at[0] = [y]
    case.read(Case.sparse(L, at), at=0)
    case.read([[x], [x]], query="xx", literal={0: (npos + 1, 2, 2) if npos >= 2 else (3, 1, 1)})
    case.read([[y], [], [x]], query="yx", literal={0: (npos, 1, 1)})
    case.figures = dict(P=L, max_pos=L - 1, n_freq_kmers=2, n_pairs=npos + 1, n_exact_pairs=npos + 1)

    def regime(ref, Wrun):
        c = ref["c"]
        assert np.bincount(c["seed_rank"]).tolist() == [npos, 1], "the row of X holds npos positions"
        assert ref["spread"][npos - 1].tolist() == ([x] if npos > 1 else [x, y]) and ref["spread"][npos].tolist() == []
        assert len(case.holders("xx", (2, 2))) == max(npos - 1, 0)
    case.regimes.append(regime)
    return case


def long_read_case():
    """A backbone read of 320 units, rank 10 + p at position p, and a second one of 40 units on the positions 100 .. 139 with the
    same ranks (f = 2: only those are frequent).  Queries: 300 units with empty clouds at the front, in the middle and at the
    end; one unit; one unit with an empty cloud; both backbone reads themselves."""
    L = 320
    case = Case("long_read", K=400, f=2, thresholds=((1, 1), (30, 30)))
    whole = case.read([[10 + p] for p in range(L)], at=0)
    part = case.read([[10 + p] for p in range(100, 140)], at=100)
    keep = [i for i in range(300) if not (i < 5 or 50 <= i < 120 or i >= 290)]
    hit = [i for i in keep if 100 <= 7 + i < 140]       # laid at 7, the units on the positions of the frequent ranks
    case.read([[10 + 7 + i] if i in set(keep) else [] for i in range(300)], query="holes", literal={0: (7, len(hit), len(hit)), 1: (-1, 0, 0)})
    case.read([[10 + 113]], query="one_unit", literal={0: (113, 1, 1), 1: (-1, 0, 0)})
    case.read([[10 + 13]], query="one_unit_rare", literal={0: (-1, 0, 0)})
    case.read([[]], query="one_empty_unit", literal={0: (-1, 0, 0)})
    case.read([[], [10 + 101], []], query="empty_ends", literal={0: (100, 1, 1)})
    case.ask(whole, "backbone_whole")
    case.ask(part, "backbone_part")
    case.literal[("backbone_whole", 0)] = case.literal[("backbone_whole", 1)] = (0, 40, 40)
    case.literal[("backbone_part", 0)] = case.literal[("backbone_part", 1)] = (100, 40, 40)
    case.figures = dict(P=L, max_pos=L - 1, n_freq_kmers=40, n_pairs=40, n_exact_pairs=40)

    def regime(ref, Wrun):
        assert len(hit) == 13 and case.units_of("holes") == 300 and case.units_of("backbone_whole") == ref["c"]["P"]
        sizes = np.diff(ref["spec"]["cloud_ptr"])[ref["spec"]["unit_ptr"][case.queries[case.q("holes")]]:][:300]
        assert sizes[:5].sum() == 0 and sizes[50:120].sum() == 0 and sizes[290:].sum() == 0 and sizes.sum() == len(keep)
        assert ref["c"]["coverage"].tolist() == [1] * 100 + [2] * 40 + [1] * 180
    case.regimes.append(regime)
    return case


# ------------------------------------------------------------------ family 4: more queries than workgroups
def stride_draw(case, n_cu, threshold=1, window=64, seed=4):
    """192 x n_cu + 5 queries drawn from the query reads of a family-1 case under its threshold (2, 2): the queries of a workgroup
    (one launch stride = 64 x n_cu apart) alternate between reads that take one window of `window` slots and reads that take two
    or more, and differ from their predecessor in read and in expected answer.  Returns (indices into case.queries, stride)."""
    ref = case.reference()
    want, span = ref["want"][threshold], ref["span"]
    windows = [-(-s // window) for s in span]
    one = [j for j, w in enumerate(windows) if w <= 1]
    many = [j for j, w in enumerate(windows) if w >= 2]
    rng = np.random.default_rng(seed)
    stride, n = 64 * n_cu, 192 * n_cu + 5
    draw = []
    for i in range(n):
        pool = many if (i // stride) % 2 else one
        while True:
            j = pool[int(rng.integers(0, len(pool)))]
            if i < stride or (case.queries[j] != case.queries[draw[i - stride]] and want[j] != want[draw[i - stride]]):
                break
        draw.append(j)
    return np.array(draw, np.int64), stride


def check_past_the_launch_cap(engine):
    """The family-1 case of 64 slots and a span of 129 starts as 192 x n_cu + 5 queries in one call, three times what the launch has
    workgroups, with map_window 64 and the default; every answer against mapcheck.  Returns figures of the run."""
    case = window_cases(64, "2W+1")
    ref = case.reference()
    for regime in case.regimes:
        regime(ref, 64)
    n_cu = engine.device_info()["n_cu"]
    t = 1
    t0, t1 = case.thresholds[t]
    draw, stride = stride_draw(case, n_cu, t)
    n = draw.size
    q = np.asarray(case.queries, np.int64)[draw]
    want = [ref["want"][t][j] for j in draw]
    windows = np.array([-(-ref["span"][j] // 64) for j in draw])
    assert n == 192 * n_cu + 5 and n > 3 * stride
    # 1: the queries of one workgroup differ from their predecessor in read and in answer
    assert (q[stride:] != q[:-stride]).all() and all(want[i] != want[i - stride] for i in range(stride, n))
    # 2: at least a quarter map and at least a quarter do not
    mapped = sum(w[0] >= 0 for w in want)
    assert 4 * mapped >= n and 4 * (n - mapped) >= n, (mapped, n)
    # 3: at least a quarter take two windows or more and follow a one-window query in their workgroup
    follow = int(((windows[stride:] >= 2) & (windows[:-stride] == 1)).sum())
    assert 4 * follow >= n, (follow, n)
    assert len({tuple(w) for w in want}) >= 8
    mapcheck.install_synthetic(engine, ref["spec"])
    engine.contig_build(ref["b_reads"], ref["b_pos"], case.f)
    assert engine.contig_info()["n_positions"] == ref["c"]["P"]
    for window in (64, 0):
        with engine.knobs(map_window=window):
            got = _triples(*engine.map_reads(q, (t0, t1)))
            bad = [i for i in range(n) if got[i] != want[i]]
            assert not bad, (f"{case.name} (window {window}): {len(bad)} of {n} queries differ from mapcheck, first at query {bad[0]} "
                             f"(the {bad[0] // stride + 1}. of its workgroup, read {list(case.q_name)[draw[bad[0]]]}): {got[bad[0]]} for {want[bad[0]]}")
    return dict(n_cu=n_cu, queries=n, workgroups=stride, mapped=mapped, several_windows_after_one=follow,
                distinct_answers=len({tuple(w) for w in want}))


# ------------------------------------------------------------------ family 5: the contig builder
def run_case(f, run, where):
    """`run` one-unit backbone reads [X] stacked on one position and a four-unit read [[1], [2], [3], [4]] on the positions 0 .. 3.
    where = first: X is rank 0 on position 0, the first sorted record; last: X is rank 5 on position 3, the last one."""
    case = Case(f"run_f{f}_{run}_{where}", K=6, f=f, thresholds=((1, 1),))
    x, p = (0, 0) if where == "first" else (5, 3)
    for _ in range(run):
        case.read([[x]], at=p)
    case.read([[1], [2], [3], [4]], at=0)
    frequent = run >= f and run >= 1
    case.read([[x]], query="x", literal={0: (p, 1, 1) if frequent else (-1, 0, 0)})
    case.read([[1], [2]], query="filler", literal={0: (0, 2, 2) if f == 1 else (-1, 0, 0)})
    n_freq = int(frequent) + (4 if f == 1 else 0)
    case.figures = dict(P=4, max_pos=3, n_freq_kmers=n_freq, n_pairs=n_freq, n_exact_pairs=n_freq)

    def regime(ref, Wrun):
        key = (ref["A"][2][:run] << 32 | p) if run else np.zeros(0, np.int64)      # the records of the stack
        assert key.size == run and (key == (x << 32 | p)).all()
        recs = np.sort(np.concatenate([key, np.array([(k << 32) | (k - 1) for k in (1, 2, 3, 4)], np.int64)]))
        if run:
            assert (recs[:run] == key).all() if where == "first" else (recs[-run:] == key).all(), "the run is the first / the last of the sorted records"
        assert run in (f - 1, f, f + 1) and ref["c"]["coverage"].tolist() == [1 + run * (q == p) for q in range(4)]
    case.regimes.append(regime)
    return case


def elsewhere_case():
    """Rank X three times on position 2 and once on position 7 under f = 3: frequent at 2, present at 7."""
    case = Case("frequent_elsewhere", K=3, f=3, thresholds=((1, 1),), spread=(0, 1, 2))
    x = 1
    for _ in range(3):
        case.read([[x]], at=2)
    case.read(Case.sparse(10, {7: [x], 0: [0], 9: [2]}), at=0)
    case.read([[x]], query="x", literal={0: (7, 1, 1)})
    case.figures = dict(P=10, max_pos=9, n_freq_kmers=1, n_pairs=2, n_exact_pairs=1)

    def regime(ref, Wrun):
        assert (ref["c"]["seed_rank"].tolist(), ref["c"]["seed_pos"].tolist()) == ([x, x], [2, 7])
        assert (ref["sc"]["exact_rank"].tolist(), ref["sc"]["exact_pos"].tolist()) == ([x], [2])
        assert ref["score"][0][0] == (2, 1, 1), "the exact scorer sees the frequent position only"
        assert ref["spread"][1].tolist() == [x] and ref["spread"][2].tolist() == []
    case.regimes.append(regime)
    return case


def f_beyond_case(f):
    """f larger than the number of records: no frequent rank, no read maps."""
    case = Case(f"f_beyond_{f}", K=4, f=f, thresholds=((1, 1), (0, 0)))
    for _ in range(5):
        case.read([[0], [1, 2]], at=0)
    case.read([[0], [1, 2]], query="same", literal={0: (-1, 0, 0), 1: (-1, 0, 0)})
    case.figures = dict(P=2, max_pos=1, n_freq_kmers=0, n_pairs=0, n_exact_pairs=0)

    def regime(ref, Wrun):
        assert f > ref["spec"]["entries"].size - 3 == 15 and ref["c"]["coverage"].tolist() == [5, 5]
    case.regimes.append(regime)
    return case


def rank_case(K, used):
    """Only one rank in use: K = 1, or rank 0 / rank K - 1 of 50."""
    case = Case(f"ranks_K{K}_{used}", K=K, f=2, thresholds=((1, 1),))
    x = 0 if used == "first" else K - 1
    case.read([[x], [], [x]], at=0)
    case.read([[x], [x]], at=0)
    case.read([[x], [x]], query="xx", literal={0: (1, 2, 2)})      # (frequent at 0, present at 1 and 2: (2, 2) at 0 and at 1 = P - 2)
    case.read([[], [x]], query="ex", literal={0: (1, 1, 1)})
    case.figures = dict(P=3, max_pos=2, n_freq_kmers=1, n_pairs=3, n_exact_pairs=1)

    def regime(ref, Wrun):
        assert np.unique(ref["spec"]["entries"]).tolist() == [x] and x in (0, K - 1)
    case.regimes.append(regime)
    return case


def key_width_case(b, c, big_pos, big_K, lead=0):
    """max_pos = 2^b - 1 or 2^b, K = 2^c or 2^c + 1.  Two copies of a three-unit read at `lead` and of a three-unit read that ends
    on max_pos, f = 2.  Rank 0 sits on the first covered position and the largest rank on the largest; rank 0 also sits next to
    the largest position and the largest rank next to the first, so that a sort that drops the top bit of the rank mixes the rows.
    lead >= 2^20: the contig begins far from 0 and P (6) is far below max_pos."""
    max_pos = (1 << b) - 1 + int(big_pos)
    K = (1 << c) + int(big_K)
    top = K - 1
    pbits, kbits = bits_that_hold(max_pos), bits_that_hold(K - 1)
    case = Case(f"key_{pbits}+{kbits}_lead{lead}", K=K, f=2, thresholds=((1, 1), (2, 2)))
    head, tail = [[0], [top, 1], [2]], [[1], [0, 2], [top]]
    for _ in range(2):
        case.read(head, at=lead)
    for _ in range(2):
        case.read(tail, at=max_pos - 2)
    at_head = lead == 0       # the mapper admits starts up to P - n = 3 only; the exact scorer goes by max_pos
    case.read(head, query="head", literal={t: (0, 3, 4) if at_head else (-1, 0, 0) for t in (0, 1)})
    case.read(tail, query="tail", literal={t: (1, 2, 2) if at_head else (-1, 0, 0) for t in (0, 1)})
    case.read([[top]], query="top", literal={0: (1, 1, 1) if at_head else (-1, 0, 0), 1: (-1, 0, 0)})
    case.read([[0]], query="zero", literal={0: (0, 1, 1) if at_head else (-1, 0, 0), 1: (-1, 0, 0)})
    case.figures = dict(P=6, max_pos=max_pos, n_freq_kmers=4, n_pairs=8, n_exact_pairs=8)
    case.width = pbits + kbits

    def regime(ref, Wrun):
        assert (pbits, kbits) == (b + int(big_pos), c + int(big_K)) and case.width == b + c + int(big_pos) + int(big_K)
        assert max_pos in ((1 << b) - 1, 1 << b) and K - 1 in ((1 << c) - 1, 1 << c)
        cc = ref["c"]
        order = np.lexsort((cc["seed_pos"], cc["seed_rank"]))
        assert (cc["seed_rank"][order[0]], cc["seed_pos"][order[0]]) == (0, lead) and (cc["seed_rank"][order[-1]], cc["seed_pos"][order[-1]]) == (top, max_pos)
        assert cc["seed_pos"][cc["seed_rank"] == 0].tolist() == [lead, max_pos - 1] and cc["seed_pos"][cc["seed_rank"] == top].tolist() == [lead + 1, max_pos]
        assert np.flatnonzero(cc["coverage"]).tolist() == [lead, lead + 1, lead + 2, max_pos - 2, max_pos - 1, max_pos]
        assert ref["score"][0][case.q("tail")] == (max_pos - 2, 3, 4) and ref["score"][0][case.q("head")] == (lead, 3, 4)
        if lead:
            assert lead >= 1 << 20 and cc["P"] * 1000 < cc["max_pos"]
    case.regimes.append(regime)
    return case


def key_width_cases():
    cases = [key_width_case(b, c, big_pos, big_K) for b, c in KEY_WIDTHS for big_pos in (False, True) for big_K in (False, True)]
    cases += [key_width_case(21, 3, big_pos, big_K, lead=(1 << 20) + 3) for big_pos in (False, True) for big_K in (False, True)]
    return cases


def record_case(n_rec, n_cu=None):
    """n_rec records from one-unit backbone reads of 64 and 65 entries (seeded), laid on n_rec // 90 positions over 128 ranks, so that
    a (rank, position) has 0.7 records on average: half of the pairs are absent, a third has one record, a sixth two or more; f = 2.
    A rank's row holds about half of the positions, so a read finds about 32 of its ranks at any start and all of them where it
    lies: the queries that are backbone reads score best on their own position with s1 = their entries (less the ranks nowhere
    frequent; a backbone read with the same cloud elsewhere ties, and the larger start wins).  The first two reads, on the first and on the last position, take their
    ranks from a second 128 that nothing else holds: present, never frequent.  n_cu: the count of the issue, 8 x n_cu x 4 x 256 + 77 records, which
    is more records than the flag kernels have threads and more reads than the emit kernel has waves."""
    K, f = 256, 2
    n_reads = n_rec // 64
    extra = n_rec - 64 * n_reads
    assert 0 <= extra <= n_reads
    npos = max(2, n_rec // 90)
    rng = np.random.default_rng(n_rec)
    sizes = np.full(n_reads, 64, np.int64)
    sizes[rng.permutation(n_reads)[:extra]] = 65
    first = rng.integers(0, 128, n_reads)
    step = 2 * rng.integers(0, 64, n_reads) + 1              # odd: 64 or 65 distinct ranks mod 128
    pos = rng.integers(0, npos, n_reads)
    pos[:npos] = np.arange(npos)                             # every position is covered: P = npos
    pos[1], pos[npos - 1] = npos - 1, 1
    owner = np.repeat(np.arange(n_reads), sizes)
    j = np.arange(n_rec) - (np.cumsum(sizes) - sizes)[owner]
    ent = (first[owner] + j * step[owner]) % 128 + 128 * (owner < 2)
    ent = ent[np.lexsort((ent, owner))]                       # every cloud ascending
    case = Case(f"records_{n_rec}", K=K, f=f, thresholds=((1, 50), (1, 1)))
    b0 = case.bulk(sizes, ent, pos)
    for name, r in (("first", b0), ("second", b0 + 1), ("middle", b0 + n_reads // 2), ("last", b0 + n_reads - 1)):
        case.ask(r, name)
    off = np.cumsum(sizes) - sizes
    case.read([ent[off[2]:off[2] + 64].tolist(), [], ent[off[3]:off[3] + 64].tolist()], query="two_clouds")
    case.figures = dict(P=npos, max_pos=npos - 1)

    def regime(ref, Wrun):
        assert ref["spec"]["entries"].size - 128 == n_rec and int(ref["c"]["coverage"].sum()) == n_reads
        assert set(sizes.tolist()) <= {64, 65} and (np.diff(ent.reshape(-1)) > 0).sum() >= n_rec - n_reads
        pair, count = np.unique((ent << 32) | pos[owner], return_counts=True)
        assert count.sum() == n_rec and count.max() >= f + 1 and (count == f).any() and (count == f - 1).any(), "runs of f - 1, f and f + 1"
        assert 0 < ref["sc"]["n_exact_pairs"] < ref["c"]["n_pairs"] < pair.size, "frequent here, frequent elsewhere, and not frequent"
        assert ref["c"]["n_freq_kmers"] <= 128 and pair.size - ref["c"]["n_pairs"] >= 128
        assert [w[0] >= 0 for w in ref["want"][1]] == [False, False, True, True, True], "the reads of rare ranks do not map, the others do"
        for t in (0, 1):
            for name, r in (("middle", n_reads // 2), ("last", n_reads - 1)):
                w = ref["want"][t][case.q(name)]      # (a rank that is nowhere frequent is one hit less; a read of the same cloud ties)
                assert w[1] == 1 and sizes[r] - 3 <= w[2] <= sizes[r] and int(pos[r]) in case.holders(name, w[1:]) and w[0] >= pos[r], \
                    "a backbone read scores best where it lies, with its entries"
        if n_cu is not None:
            assert n_rec == 8 * n_cu * 4 * 256 + 77 and n_reads > 8 * n_cu * 4 * 4
    case.regimes.append(regime)
    return case


def coverage_case():
    """299 one-unit reads on position 5, every other one with an empty cloud, and one read over 0 .. 10."""
    case = Case("coverage_300", K=4, f=150, thresholds=((1, 1),))
    for j in range(299):
        case.read([[1] if j % 2 == 0 else []], at=5)
    case.read([[0]] + [[]] * 9 + [[2]], at=0)
    case.read([[1]], query="x", literal={0: (5, 1, 1)})
    case.read([[0]], query="rare", literal={0: (-1, 0, 0)})
    case.figures = dict(P=11, max_pos=10, n_freq_kmers=1, n_pairs=1, n_exact_pairs=1)

    def regime(ref, Wrun):
        assert ref["c"]["coverage"].tolist() == [1] * 5 + [300] + [1] * 5, "empty clouds cover too"
        assert int(np.count_nonzero(np.diff(ref["spec"]["cloud_ptr"])[:299])) == 150 == case.f
    case.regimes.append(regime)
    return case


def check_runs(engine, f):
    for run in (f - 1, f, f + 1):
        for where in ("first", "last"):
            check(engine, run_case(f, run, where), reverse=True)


def check_key_widths(engine):
    cases = key_width_cases()
    widths = sorted({c.width for c in cases})
    assert set(widths) >= {8, 9, 16, 17, 24, 25}, widths
    assert sum(1 for c in cases if not c.name.endswith("_lead0")) == 4, "four cases begin at 2^20 + 3"
    for case in cases:
        check(engine, case, reverse=True)
    return widths


def check_record_count(engine, n_rec):
    return check(engine, record_case(n_rec), reverse=True)


def check_more_records_than_threads(engine):
    n_cu = engine.device_info()["n_cu"]
    case = record_case(8 * n_cu * 4 * 256 + 77, n_cu)
    ref = check(engine, case)
    return dict(n_cu=n_cu, records=int(ref["spec"]["entries"].size - 128), backbone_reads=len(case.backbone), n_pairs=ref["c"]["n_pairs"],
                n_exact_pairs=ref["sc"]["n_exact_pairs"], positions=ref["c"]["P"])

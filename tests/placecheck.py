"""cf_place_reads (cf_place2.hip, cf_place.hip) on hand-built clouds at the capacities of its kernels: the case builders, a traced
restatement of the placement and the case bodies shared by the emulator and the GPU suite (test_emu_place_shapes.py,
test_gpu_place_shapes.py).

A case is written straight as clouds of k-mer ranks — reads of one base per unit, ranks 0 .. K - 1 through set_kmers, then set_clouds
(mapcheck.synthetic_arrays does the same) — so that it decides which branch of the kernels runs, not the sequence it came from.
Every expected line comes from oracle.placer.place_reads (oracle.cport.place_reads, which test_cport_is_the_python_oracle pins to it
on every small case, only where a case says so).  The comparison is exact, every line, through conftest.lines_from_placement with
ids that sort as id_rank does; the ranks are a seeded permutation of record order.

trace() is a second restatement that shares no code with the kernels nor with oracle.placer (scores as the reference keeps them, a
counter per (read, offset, unit); the contig per k-mer): every body asserts it line-equal to the oracle and takes from it — never
from the library — the figures that show the case is where it claims to be: per tail the reads with a hit on a hot row ("dirty"),
their blocks of 64 and their hot rows, per event of a laid read the stage postings of its k-mer, per k-mer its contig positions, the
largest counter, the offsets per read.  The capacity a case aims at stands as a literal next to the assertion, the kernel constant
in a comment.

A tail: the seed of a stage (tail 0) and every greedy iteration (tail t = after the t-th read of the stage was laid down).
hot = max(1, min_inters): a score row with that many hits can qualify; only hits on such rows make a read dirty."""
import numpy as np

from conftest import lines_from_placement
from oracle import placer

MODES = (1, 2, 3)


# ------------------------------------------------------------------ cases
class Case:
    """reads: [(class, [cloud, ...])], a cloud = a list of distinct ranks < K.  params = (min_cloud_kmer_freq, min_unit, min_inters,
    min_prop).  rank: "shuffled" (seeded permutation), "reversed" or an explicit list.  small: plain Python restates it in well
    under a second (the cport pin runs on these)."""

    def __init__(self, name, reads, K, params, rank="shuffled", knobs=None, small=True):
        self.name, self.K, self.params, self.knobs, self.small = name, int(K), tuple(params), dict(knobs or {}), small
        R = len(reads)
        self.classes = np.array([c for c, _ in reads], np.uint8)
        n_units = [len(u) for _, u in reads]
        self.unit_ptr = np.concatenate([[0], np.cumsum(n_units)]).astype(np.int64)
        sizes = [len(c) for _, u in reads for c in u]
        self.cloud_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        flat = [np.asarray(c, np.int32) for _, u in reads for c in u if len(c)]
        self.entries = np.concatenate(flat).astype(np.int32) if flat else np.zeros(0, np.int32)
        assert self.entries.size == 0 or (0 <= int(self.entries.min()) and int(self.entries.max()) < self.K), name
        if isinstance(rank, str):
            rng = np.random.default_rng(sum(map(ord, name)))
            self.id_rank = {"shuffled": rng.permutation(R), "reversed": np.arange(R)[::-1]}[rank].astype(np.int32)
        else:
            self.id_rank = np.asarray(rank, np.int32)
        assert sorted(self.id_rank.tolist()) == list(range(R)), name
        assert R < 3 or not np.array_equal(self.id_rank, np.arange(R)), f"{name}: the ranks repeat record order"
        self.ids = [f"r{int(k):07d}" for k in self.id_rank]      # ascending string order IS id_rank
        self._want = self._trace = None

    def arrays(self):
        return self.unit_ptr, self.cloud_ptr, self.entries, self.K, self.classes, self.id_rank, self.params

    def want(self):
        """The oracle's lines, computed once per case."""
        if self._want is None:
            self._want = placer.place_reads(self.ids, self.classes.astype(np.int64), self.unit_ptr, self.cloud_ptr, self.entries.astype(np.int64), *self.params)
        return self._want

    def want_cport(self):
        from oracle import cport
        return lines_from_placement(self.ids, *[x.tolist() for x in cport.place_reads(self.classes, self.id_rank, self.unit_ptr, self.cloud_ptr, self.entries, self.K, *self.params)])

    def traced(self):
        if self._trace is None:
            self._trace = trace(self)
            assert self._trace["lines"] == self.want(), f"{self.name}: the traced restatement and oracle.placer disagree"
        return self._trace


# ------------------------------------------------------------------ the traced restatement
def trace(case):
    f, min_unit, min_inters, min_prop = case.params
    thr, hot = max(1, int(f)), max(1, int(min_inters))
    up, cp, ent = case.unit_ptr.tolist(), case.cloud_ptr.tolist(), case.entries.tolist()
    rank, ids, cls = case.id_rank.tolist(), case.ids, case.classes.tolist()
    R = len(cls)
    units = [[ent[cp[u]:cp[u + 1]] for u in range(up[r], up[r + 1])] for r in range(R)]
    where = {}                      # k-mer -> {position: count}, positions in the order they were first laid
    frequent = {}                   # k-mer -> True, in the order they became frequent
    fig = dict(lines=[], tails=[], event_postings=[], event_ordinal=[], max_counter=0, seed_below_thr=[], qualifying=[], offsets={})

    def lay(r, pos):
        fired = []
        for i, cloud in enumerate(units[r]):
            for x in cloud:
                at = where.setdefault(x, {})
                at[pos + i] = at.get(pos + i, 0) + 1
                if at[pos + i] == thr:
                    frequent[x] = True
                    fired.append((x, pos + i, list(at).index(pos + i)))
        return fired

    for r in range(R):
        if cls[r] == 0:
            lay(r, 0)
            fig["lines"].append(f"{ids[r]} 0")
    for stage in (1, 2):
        members = [r for r in range(R) if cls[r] == stage]
        holders = {}                # k-mer -> [(read, unit index)] among the stage's reads
        for r in members:
            for i, cloud in enumerate(units[r]):
                for x in cloud:
                    holders.setdefault(x, []).append((r, i))
        score = {r: {} for r in members}      # read -> offset -> unit index -> hits
        left = set(members)
        pending = [(x, q, None) for x in frequent for q in where[x]]
        fig["seed_below_thr"].append(sum(1 for x, q, _ in pending if where[x][q] < thr))
        laid = False
        while left:
            touched = set()
            for x, q, ordinal in pending:
                if laid:
                    fig["event_postings"].append(len(holders.get(x, ())))
                    fig["event_ordinal"].append(ordinal)
                for r, i in holders.get(x, ()):
                    if q < i:
                        continue
                    row = score[r].setdefault(q - i, {})
                    row[i] = row.get(i, 0) + 1
                    if row[i] > fig["max_counter"]:
                        fig["max_counter"] = row[i]
                    touched.add((r, q - i))
            dirty = {r for r, off in touched if sum(score[r][off].values()) >= hot}
            fig["tails"].append(dict(stage=stage, dirty=len(dirty), blocks=len({r >> 6 for r in dirty}),
                                     hot_rows={r: sum(1 for row in score[r].values() if sum(row.values()) >= hot) for r in dirty}))
            best, ok = None, set()
            for r in left:
                for off, row in score[r].items():
                    s0, s1 = len(row), sum(row.values())
                    if s0 >= min_unit and s0 * min_prop <= s1 and s1 >= min_inters:
                        ok.add(r)
                        key = (s0, s1, off, -rank[r])
                        if best is None or key > best[0]:
                            best = (key, r)
            fig["qualifying"].append(ok)
            if best is None:
                fig["lines"].extend(f"{ids[r]} None" for r in sorted(left, key=lambda r: rank[r]))
                break
            (s0, s1, off, _), r = best
            fig["lines"].append(f"{ids[r]} {off} {s0} {s1}")
            pending = lay(r, off)
            laid = True
            left.discard(r)
        fig["offsets"].update({r: len(score[r]) for r in members})
    fig["positions"] = {x: len(at) for x, at in where.items()}
    return fig


# ------------------------------------------------------------------ running a case on an engine
def install(engine, case):
    up = case.unit_ptr
    U = int(up[-1])
    engine.load_arrays(np.full(U, ord("A"), np.uint8), up, up, np.arange(U, dtype=np.int64), np.arange(U, dtype=np.int64) + 1)
    engine.set_kmers(np.arange(case.K, dtype=np.uint64), 16)
    engine.set_clouds(case.cloud_ptr, case.entries)


def run(engine, case, mode, knobs=None, installed=False):
    """The library's lines for the case under place_mode `mode`.  Mode 2 keeps the regions however many long rescans the case makes
    (place_long_rescans: the default hands such runs to the hash-map path, which mode 1 runs anyway)."""
    if not installed:
        install(engine, case)
    k = dict(case.knobs, **(knobs or {}))
    k["place_mode"] = mode
    k.setdefault("place_long_rescans", 1000000)
    with engine.knobs(**k):
        out = engine.place_reads(case.classes, case.id_rank, *case.params)
    return lines_from_placement(case.ids, *[x.tolist() for x in out])


def check(engine, case, modes=MODES, knobs=None):
    """Every line of the case on every mode against the oracle; returns the traced figures."""
    fig = case.traced()
    want = case.want()
    install(engine, case)
    for mode in modes:
        got = run(engine, case, mode, knobs, installed=True)
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert len(got) == len(want) and not bad, f"{case.name} mode {mode} {knobs or ''}: {len(bad)} of {len(want)} lines differ, first {bad[:3]}"
    return fig


def ranks(first, n):
    return list(range(first, first + n))


# ------------------------------------------------------------------ posting rows
POSTING_COUNTS = (31, 32, 63, 64, 65, 200)


def posting_two(n):
    """The postings (0 = L) of the two-unit holders of X among n.  The last word of a posting row is the k-mer's posting COUNT: taken for
    a posting it would name read n >> 2, unit n & 3 (ib = 2 bits of unit index) — for n = 32, 64 and 200 unit 0 of a read that holds X
    there, and that read is one of the two-unit ones (reads 0 and 1 are the prefix read and L: posting p belongs to read p + 1)."""
    return {p for p in (1, 30, 31, 62, 63, 64, n - 1, (n >> 2) - 1 if n >= 32 and n % 4 == 0 else 0) if 0 < p < n}


def posting_case(n):
    """K-mer X with exactly n postings among the internal reads; the read L that the seed places (two units on the prefix read)
    brings X, Y0 .. Y2 to position 2 and W to position 3 for the first time: with a threshold of 1 each raises an event in the first
    greedy iteration.  The other holders of X:
      two-unit reads [X Y0 Y1 Y2][W]  they reach s1 = 5 = min_inters at offset 2 ONLY with X's hit, and are placed (by rank)
      one-unit reads [X Y0 Y1 Y2]     four hits, never placed (min_unit 2): the postings in between
      four-unit reads [] [] [] [X]    q = 2 < i = 3: dropped postings
    in posting order (the emulator fills the lists in read order; on hardware the order inside a list is whatever the atomics made it):
    the two-unit ones at postings 1, 30, 31, 62, 63, 64, n - 1 where they exist (posting_two), a dropped one at 5 (the row part) and at
    every fourth from 66 on (the continuation)."""
    A = ranks(0, 8)
    X, Y, W = 8, ranks(9, 3), 12
    reads = [(0, [A[:4], A[4:]]), (1, [A[:4], A[4:], [X] + Y, [W]])]
    two = posting_two(n)
    for p in range(1, n):
        if p in two:
            reads.append((1, [[X] + Y, [W]]))
        elif p == 5 or (p >= 66 and p % 4 == 2):
            reads.append((1, [[], [], [], [X]]))
        else:
            reads.append((1, [[X] + Y]))
    reads.append((1, [[W], []]))      # holds W only: never hot
    return Case(f"postings_{n}", reads, 16, (1, 2, 5, 1))


def check_posting_rows(engine, n, knobs=None):
    case = posting_case(n)
    fig = check(engine, case, knobs=knobs)
    # rows hold 31 postings (32 words) or 63 (64 words: from 32 postings on), the rest comes from the CSR lists (the 64th on)
    assert max(fig["event_postings"]) == n, fig["event_postings"]      # PW - 1 = 31 / 63 (cf_pl2_iter_kernel)
    placed = [ln for ln in fig["lines"] if ln.endswith(" 2 2 5")]
    assert len(placed) == len(posting_two(n)), placed
    return fig


# ------------------------------------------------------------------ the dirty list
DIRTY_COUNTS = (1, 63, 64, 65, 2047, 2048, 2049, 5000)


def dirty_case(n, by):
    """n reads made dirty by ONE tail: by the seed's (by = "seed": their unit lies on the prefix read) or by the first greedy
    iteration's (by = "laid": on units 2 and 3 of the read that the seed places, new to the contig).  min_inters 4 = the four k-mers of
    a unit, so every hit row is hot.  All but six are one-unit reads, never placed; three two-unit reads at either end of the read
    numbers are — those at the far end only if the words of the dirty bitmap that did not fit the list are kept for the next round."""
    a, b, c, d = ranks(0, 4), ranks(4, 4), ranks(8, 4), ranks(12, 4)
    if by == "seed":
        reads, tail = [(0, [a, b])], n
    else:
        reads, tail = [(0, [c, d]), (1, [c, d, a, b])], n - 1      # (the laid read receives its own hits: it is one of the n)
    n_two = min(3, tail // 2)
    for j in range(tail):
        reads.append((1, [a, b] if j < n_two or j >= tail - n_two else [a]))
    reads.append((1, [ranks(16, 4)]))      # hits nothing
    return Case(f"dirty_{by}_{n}", reads, 24, (1, 2, 4, 1), small=n <= 100)


def check_dirty_list(engine, n, by, modes=MODES):
    case = dirty_case(n, by)
    fig = check(engine, case, modes)
    t = fig["tails"][0 if by == "seed" else 1]
    assert t["dirty"] == n, (t["dirty"], n)      # PL2_LIST = 2048 reads per round of the tail
    assert t["blocks"] >= (n + 63) // 64      # blocks of 64 reads; the last one is not full (the read count is no multiple of 64)
    assert case.classes.size % 64 != 0
    return fig


def touched_blocks_case(n_blocks=600, n_reads=600 * 64 + 5):
    """At least 513 touched blocks of 64 reads in a single-round tail (m > PL2_CRES: the sweep is not fused): one dirty read in each of
    n_blocks blocks — 600 <= 2048, one round — of a read set of more than 32 768 reads; the others hold a k-mer nobody lays down.
    Four of the dirty reads have a second unit and are placed."""
    a, b = ranks(0, 4), ranks(4, 4)
    reads = [(0, [a, b])]
    for r in range(1, n_reads):
        if r % 64 == 7 and r // 64 < n_blocks:
            reads.append((1, [a, b] if r // 64 in (0, 300, 511, 599) else [a]))
        else:
            reads.append((1, [[9]]))
    return Case("touched_blocks", reads, 10, (1, 2, 4, 1), small=False)


def check_touched_blocks(engine, modes=MODES):
    case = touched_blocks_case()
    fig = check(engine, case, modes)
    t = fig["tails"][0]
    assert t["dirty"] == 600 and t["dirty"] <= 2048      # PL2_LIST: one round
    assert t["blocks"] == 600 and t["blocks"] >= 513      # PL2_CRES = 512
    assert case.classes.size >= 32769
    return fig


# ------------------------------------------------------------------ heavy reads
HOT_ROW_COUNTS = (4, 5, 6, 512, 513, 1100)


def heavy_spots(n_rows):
    """The prefix units p whose b_p a two-unit read holds (its best row is offset p - 1): every one of 1 .. n_rows up to eight rows,
    else seven spread evenly and the last."""
    return list(range(1, n_rows + 1)) if n_rows <= 8 else sorted({1 + (j * (n_rows - 2)) // 6 for j in range(7)} | {n_rows})


def heavy_case(n_rows, n_reads=None, name=None):
    """Reads with n_rows hot rows after the seed: the prefix read has n_rows units [a0 a1 b_p] and a last one [b_p] alone; a read
    [a0 a1][b_p] meets a0 a1 at every offset 0 .. n_rows - 1 (two hits = min_inters: a hot row each) and qualifies at offset p - 1
    alone (s0 = 2, s1 = 3).  One such read per p of heavy_spots at the front of the read numbers and one at the back; one-unit reads
    [a0 a1] — as many hot rows, never placed — in between.  All two-unit reads have regions of one size, so an offset has the same
    slot in each of them: with EVERY offset the best row of some read (up to eight rows) the fifth row that a rescan meets, the
    sixth, ... each decide a line, whichever offsets the hash puts there; beyond, the spread puts best rows behind the 512th."""
    a = [0, 1]
    prefix = [a + [2 + p] for p in range(n_rows)] + [[2 + n_rows]]
    spots = heavy_spots(n_rows)
    n_reads = n_reads or 2 * len(spots)
    reads = [(0, prefix)]
    for j in range(n_reads):
        front, back = j < len(spots), n_reads - 1 - j < len(spots)
        if front or back:
            reads.append((1, [a, [2 + (spots[j] if front else spots[n_reads - 1 - j])]]))
        else:
            reads.append((1, [a]))
    return Case(name or f"heavy_{n_rows}", reads, 3 + n_rows, (1, 2, 2, 1), small=n_rows <= 16)


def check_heavy_rows(engine, n_rows, modes=MODES):
    case = heavy_case(n_rows)
    fig = check(engine, case, modes)
    rows = fig["tails"][0]["hot_rows"]
    # a lane rescans a read with up to four hot rows besides its anchor, a wave those with more, PL2_HSCR = 512 rows per pass
    assert max(rows.values()) == n_rows and min(rows.values()) >= n_rows - 1, sorted(set(rows.values()))
    assert sum(1 for ln in fig["lines"] if ln.endswith(" 2 3")) == 2 * len(heavy_spots(n_rows)) >= 8
    return fig


def check_many_heavy_reads(engine, modes=MODES):
    """More than 512 reads with more than four hot rows in ONE tail: the heavy list (PL2_HEAVY = 512) is full and the lanes walk the
    rest of their reads' rows themselves."""
    case = heavy_case(8, n_reads=540, name="heavy_reads_540")
    fig = check(engine, case, modes)
    rows = fig["tails"][0]["hot_rows"]
    assert sum(1 for n in rows.values() if n > 5) == 540 and 540 > 512      # PL2_HEAVY (n > 5: more than four besides an anchor, whichever row that is)
    assert sum(1 for ln in fig["lines"] if ln.endswith(" 2 3")) == 16      # eight at either end: every one of the eight offsets is some read's best row
    return fig


# ------------------------------------------------------------------ contig records
def contig_case(n_pos, f):
    """K-mer X at n_pos contig positions: 0 .. 2 by f prefix reads PA (frequent from the start, with the g k-mers that place L1 and L2),
    3 .. n_pos - 1 by f - 1 prefix reads PB — position 3 takes the record's fourth word, the others live in the overflow map, at count
    f - 1 — and by the internal reads L1 and L2, which hold X in EVERY unit from 3 on (several claims on one record in one launch): L1
    brings each of those pairs to the threshold exactly, L2 past it (no second event).  Readers [X][X], [X][X][X] and [][X] collect
    what was raised: a hit too many or too few changes their s1."""
    X, g = 0, [[1 + 2 * u, 2 + 2 * u] for u in range(4)]
    PA = [[X] + g[u] if u < 3 else g[u] for u in range(4)]
    PB = [[] for _ in range(3)] + [[X] for _ in range(3, n_pos)]
    L = [g[0], g[1], g[2], [X] + g[3]] + [[X] for _ in range(4, n_pos)]
    reads = [(0, PA)] * f + [(0, PB)] * (f - 1) + [(1, L), (1, [[X], [X]]), (1, L), (1, [[X], [X], [X]]), (1, [[], [X]]), (2, [[X], [X]]), (2, L)]
    return Case(f"contig_{n_pos}_{f}", reads, 10, (f, 2, 2, 1), knobs={"place_cmap_bits": 3})


def check_contig_records(engine, n_pos, f, modes=MODES):
    case = contig_case(n_pos, f)
    fig = check(engine, case, modes)
    assert fig["positions"][0] >= n_pos      # a record holds four positions (cf_pl2_crec), the fifth goes to the map
    if n_pos > 4:
        assert max(o for o in fig["event_ordinal"] if o is not None) >= 4, fig["event_ordinal"]      # an event from the overflow map
        assert n_pos < 9 or fig["positions"][0] - 4 > 4      # place_cmap_bits 3: 8 slots, grown past half load
    assert fig["seed_below_thr"][0] > 0 or f == 1      # f >= 2: the seed takes in the pairs of X that are below the threshold
    return fig


# ------------------------------------------------------------------ score regions
def region_case(when, n_off=100):
    """A one-unit read [a] that meets n_off offsets (a region of one unit starts with 64 slots) at the seed — the prefix read holds a in
    n_off units — or during the first iteration — the read L that the seed places does.  [a][a] is placed behind it."""
    g, a = [[1, 2], [3, 4]], [0]
    if when == "seed":
        reads = [(0, g + [a] * n_off), (1, [a]), (1, [a, a]), (1, [[5]])]
    else:
        reads = [(0, g), (1, g + [a] * n_off), (1, [a]), (1, [a, a]), (1, [[5]])]
    return Case(f"region_{when}_{n_off}", reads, 6, (1, 2, 2, 1))


def check_score_regions(engine, when, knobs=None, modes=MODES):
    case = region_case(when)
    fig = check(engine, case, modes, knobs)
    assert max(fig["offsets"].values()) > 64      # 64 slots: the smallest region (pl2_attempt)
    return fig


UNIT_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)


def random_case(max_units, seed, K=60, n_reads=26):
    """Seeded reads off a made-up array of max_units + 3 positions with a cloud of five ranks out of K - 5 each (so a rank sits at several
    positions; the last five ranks are used by nobody): a read is a window of the array, every k-mer kept with probability 0.7 (all of them in a prefix read), a
    stray one added now and then, an empty cloud now and then.  The longest read has max_units units, the first reads have every
    length below it down to none; two prefix reads at the array's start, internal and suffix reads mixed."""
    rng = np.random.default_rng(1000 * max_units + seed)
    array = [rng.choice(K - 5, 5, replace=False).tolist() for _ in range(max_units + 3)]
    reads = []
    for r in range(n_reads):
        n = max_units - r if r <= max_units else int(rng.integers(1, max_units + 1))
        cls = 0 if r in (0, max_units + 2) else int(rng.choice([1, 1, 1, 2]))
        start = 0 if cls == 0 else int(rng.integers(0, max_units + 3 - n + 1))
        units = []
        for i in range(n):
            cloud = [x for x in array[start + i] if cls == 0 or rng.random() < 0.7]
            if rng.random() < 0.2:
                cloud.append(int(rng.integers(0, K - 5)))
            units.append(sorted(set(cloud)) if rng.random() < 0.9 else [])
        reads.append((cls, units))
    f, mu, mi, mp = [(1, 2, 2, 1), (2, 2, 4, 1), (1, 1, 1, 0), (2, 2, 3, 1), (1, 2, 5, 2)][seed % 5]
    if max_units == 1:
        mu, mi, mp = 1, min(mi, 3), min(mp, 1)
    return Case(f"random_{max_units}_{seed}", reads, K, (f, mu, mi, mp))


def check_unit_counts(engine, max_units, modes=MODES):
    figs = []
    for seed in range(5):
        case = random_case(max_units, seed)
        figs.append(check(engine, case, modes))
        assert int(np.diff(case.unit_ptr).max()) == max_units      # ib = 1, 1, 2, 2, 3, 3, 3, 4 bits of unit index (cf_place2_fits)
    assert sum(1 for f in figs if sum(1 for ln in f["lines"] if ln.count(" ") == 3) >= 3) >= 3, "too few reads placed to tell anything"
    return figs


# ------------------------------------------------------------------ order and thresholds
def ties_case(rank):
    """66 reads [g0 g1][g2 g3] tied on (2, 4, offset 0) in three blocks of 64 reads, one-unit reads between them: placed by rank."""
    g = [[0, 1], [2, 3]]
    reads = [(0, g)]
    for r in range(1, 150):
        reads.append((1, g if r % 2 == 0 and sum(1 for c, u in reads if len(u) == 2) <= 66 else [g[0]]))
    return Case(f"ties_{rank}", reads, 4, (1, 2, 4, 1), rank=rank)


def check_ties(engine, rank, modes=MODES):
    case = ties_case(rank)
    fig = check(engine, case, modes)
    tied = [ln for ln in fig["lines"] if ln.endswith(" 0 2 4")]
    assert len(tied) == 66 > 64 and len({r >> 6 for r in range(1, 150) if case.unit_ptr[r + 1] - case.unit_ptr[r] == 2}) == 3
    assert [ln.split()[0] for ln in tied] == sorted(ln.split()[0] for ln in tied)
    return fig


def offset_beats_id_case():
    """Two reads tied on (s0, s1) = (2, 4): the one at offset 3 is placed first although the other has the smaller id."""
    g, h = [[0, 1], [2, 3]], [[4, 5], [6, 7]]
    return Case("offset_beats_id", [(0, g + [[]] + h), (1, h), (1, g)], 8, (1, 2, 4, 1), rank=[1, 2, 0])


def threshold_case(min_prop):
    """min_unit 2, min_inters 6, min_prop 3 (then 1 and 0): reads whose best row is (s0, s1) = (2, 6) or (3, 9) — every threshold met
    exactly — and one short of each: (1, 6) of min_unit, (2, 5) of min_inters, (3, 8) of s0 * min_prop <= s1 alone (9 > 8), (3, 6) too."""
    P = [ranks(0, 6), ranks(6, 6), ranks(12, 6)]
    reads = [(0, P),
             (1, [P[0][:3], P[1][:3]]),                # 2, 6
             (1, [P[0]]),                              # 1, 6
             (1, [P[0][:3], P[1][:2]]),                # 2, 5
             (1, [P[0][:2], P[1][:2], P[2][:2]]),      # 3, 6
             (1, [P[0][:4], P[1][:2]]),                # 2, 6 again
             (1, [P[0][:3], P[1][:3], P[2][:2]]),      # 3, 8
             (1, [P[0][:3], P[1][:3], P[2][:3]]),      # 3, 9
             (1, [P[0][:1], P[1][:1]])]                # 2, 2
    return Case(f"thresholds_prop{min_prop}", reads, 18, (1, 2, 6, min_prop))


def requalify_case():
    """A read that qualifies, stops qualifying because s0 grows, and qualifies again (s0 * min_prop <= s1 is not monotone; min_prop 3).
    Prefix read [] [] v0 v1 p q w (three ranks each).  At the seed W = [p q w+x] has (3, 9) at offset 4, Q = [p+y q x] (2, 6) at offset
    4 and V = [v0 v1 y] (2, 6) at offset 2.  W is placed and brings x to position 6: Q has (3, 7), 9 > 7.  Q's record of the seed would
    still beat V by its offset; V is placed and brings the five y to position 4: Q has (3, 12) and is placed."""
    v0, v1, p, q, w = (ranks(3 * j, 3) for j in range(5))
    x, y = 15, ranks(16, 5)
    reads = [(0, [[], [], v0, v1, p, q, w]), (1, [p + y, q, [x]]), (1, [p, q, w + [x]]), (1, [v0, v1, y]), (1, [[21]])]
    return Case("requalify", reads, 22, (1, 2, 6, 3), rank=[4, 0, 3, 2, 1])


# ------------------------------------------------------------------ stages
def stage_cases():
    g = [[0, 1], [2, 3]]
    two = [(0, g), (0, g)]
    return [
        # the reference's over-inclusive seed: X = 4 is frequent at position 0 (two prefix reads); the internal read lays it at position 3
        # ONCE (count 1 < 2) — the suffix stage's seed takes (X, 3) in all the same: the suffix read [g0 g1][g2 g3][][X] has (3, 5), not (2, 4)
        Case("suffix_seed_over_inclusive", [(0, [[4] + g[0], g[1]]), (0, [[4] + g[0], g[1]]), (1, g + [[], [4]]), (2, g + [[], [4]]), (2, [[4]])], 5, (2, 2, 2, 1)),
        Case("no_internal_reads", two + [(2, g), (2, [g[0]]), (2, g)], 4, (2, 2, 4, 1)),
        Case("no_suffix_reads", two + [(1, g), (1, [g[0]]), (1, g)], 4, (2, 2, 4, 1)),
        Case("only_suffix_reads_no_prefix", [(2, g), (2, g), (2, [g[0]])], 4, (1, 2, 4, 1)),
        Case("no_prefix_read", [(1, g), (2, g), (1, [g[0]]), (2, g), (1, g)], 4, (1, 2, 4, 1)),
        Case("reads_without_units", [(1, []), (0, g), (1, []), (1, g), (2, []), (1, [[], []]), (2, g), (0, []), (1, g)], 4, (1, 2, 4, 1)),
        Case("empty_clouds_and_unused_ranks", [(0, [[], [100, 101], [], [300, 301]]), (1, [[], [100, 101], [], [300, 301], []]), (1, [[100, 101], [], [300, 301]]),
                                               (2, [[], [], [300, 301], [499]]), (1, [[], []])], 500, (1, 2, 4, 1)),
        Case("one_read", [(1, g)], 4, (1, 2, 4, 1), rank=[0]),
        Case("one_prefix_read", [(0, g)], 4, (1, 2, 4, 1), rank=[0]),
    ]


def small_cases():
    """Every case of this file that plain Python restates quickly: the cport pin and the bodies of the small tests run on them."""
    out = [posting_case(n) for n in POSTING_COUNTS]
    out += [dirty_case(n, by) for n in DIRTY_COUNTS if n <= 100 for by in ("seed", "laid")]
    out += [heavy_case(n) for n in HOT_ROW_COUNTS if n <= 16]
    out += [contig_case(n, f) for n in (4, 5, 9) for f in (1, 2, 3)]
    out += [region_case("seed"), region_case("laid")]
    out += [random_case(u, s) for u in UNIT_COUNTS for s in range(5)]
    out += [ties_case("shuffled"), ties_case("reversed"), offset_beats_id_case(), requalify_case()]
    out += [threshold_case(p) for p in (3, 1, 0)]
    out += stage_cases()
    return out


def check_order_and_thresholds(engine, modes=MODES):
    fig = check(engine, offset_beats_id_case(), modes)
    assert fig["lines"][1].endswith(" 3 2 4") and fig["lines"][2].endswith(" 0 2 4") and fig["lines"][1] > fig["lines"][2], fig["lines"]
    for min_prop, n_placed in ((3, 3), (1, 5), (0, 5)):
        fig = check(engine, threshold_case(min_prop), modes)
        placed = [ln for ln in fig["lines"][1:] if not ln.endswith("None")]
        assert len(placed) == n_placed, (min_prop, fig["lines"])      # prop 3: (3, 9) and the two (2, 6); prop 1 and 0: (3, 8) and (3, 6) too
    case = requalify_case()
    fig = check(engine, case, modes)
    assert [1 in ok for ok in fig["qualifying"][:3]] == [True, False, True]      # read 1 = Q: qualifies, stops, qualifies again
    assert [ln.split(" ", 1)[1] for ln in fig["lines"][1:4]] == ["4 3 9", "2 2 6", "4 3 12"], fig["lines"]
    return fig


def check_stages(engine, modes=MODES):
    for case in stage_cases():
        fig = check(engine, case, modes)
        if case.name == "suffix_seed_over_inclusive":
            assert fig["seed_below_thr"][1] >= 1 and fig["lines"][-2].endswith(" 0 3 5"), fig["lines"]
        if case.name in ("only_suffix_reads_no_prefix", "no_prefix_read"):
            assert all(ln.endswith(" None") for ln in fig["lines"])      # (per stage in rank order: the oracle's lines say so)


# ------------------------------------------------------------------ clouds larger than their units
def big_cloud_case(n):
    """Clouds of n entries on units of ONE base: C = ranks 0 .. n - 1, D = the next 20.  r2 [C D] is placed first, at offset 0 on
    the prefix reads r0 [C D . . . C] and r1 [. D . . . C]; r3 [C D] then holds 2 n hits in the counter of (r3, offset 0, unit 0) —
    n from the seed, n more from the pairs (C, 0) that r2 brought to the threshold of 2 — and is placed with s1 = 2 n + 20."""
    C_, D_ = ranks(0, n), ranks(n, 20)
    reads = [(0, [C_, D_, [], [], [], C_]), (0, [[], D_, [], [], [], C_]), (1, [C_, D_]), (1, [C_, D_])]
    return Case(f"big_cloud_{n}", reads, n + 20, (2, 1, 10, 1), rank=[1, 0, 3, 2], small=False)


BIG_CLOUDS = (32767, 32768, 33000)


def check_big_clouds(engine, n):
    """Modes 1 and 2: the oracle's lines (the default path notices that a 16-bit cell cannot count such a cloud and takes the hash-map
    path).  Mode 3: the same while 2 n fits 16 bits (n = 32 767), else -34 with the reason."""
    from centroflye_amd.engine import DeviceError
    import pytest
    case = big_cloud_case(n)
    fig = check(engine, case, (1, 2))
    assert fig["max_counter"] == 2 * n      # a score cell has 16 bits: 65 535 (cf_pl2_rinfo: two cells per word)
    assert fig["lines"][-1].endswith(f" 0 2 {2 * n + 20}"), fig["lines"]
    if 2 * n <= 65535:
        check(engine, case, (3,))
    else:
        with pytest.raises(DeviceError, match=r"\(-34\).*cloud of " + str(n) + " entries"):
            run(engine, case, 3)
    return fig

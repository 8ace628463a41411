"""Stages A1-A6 on hand-built reads at the kernels' shape boundaries, against a plain restatement on Python byte strings.

Every other differential test feeds the device the output of a generator of centromeric reads: k in 9 .. 31, units of hundreds
to thousands of bases, clouds of 100 - 450 ranks.  The kernels switch code paths on shape just outside that band:
  * cf_cloud_kernel ranks a cloud of up to 512 entries by counting smaller ones, sorts 513 .. 1536 with the bitonic network in
    its 2048-slot LDS set, repeats the whole launch with the 8192-slot set from 1537, refuses beyond 6144 (-34), and stages a
    unit in tiles of 2048 windows;
  * A1's first pass reads a tile's bases as aligned 32-bit words at a byte offset 0 .. 3, patches the last word of the base
    array byte by byte, cuts reads into tiles of 4096 windows and takes windows out of a 128-bit shift that depends on k;
  * the multi-occurrence cut at one, two and three reads (read bits 0 / 1 / 2 in the record);
  * the distance stage on dense clouds (hundreds of ranks per unit out of a small set);
  * the radix sort on a grid that strides.
naive_stage2 below is the reference's algorithm on bytes, dicts and sets; it shares no code with oracle/recruit.py or the
kernels (test_emu_shapes.py pins it to the oracle on the `tiny` fixture).  Every case carries a `regime` check that is
evaluated on the naive result alone, BEFORE the device runs: a case that drifted out of the branch it was built for fails.
All comparisons are integer-exact.  Used by test_emu_shapes.py (host emulator) and test_gpu_shapes.py (MI355X)."""
import math
from collections import Counter, defaultdict

import numpy as np

import pathcheck
from centroflye_amd.engine import DeviceError

TILE = 4096                   # keys per radix tile (cf_radix.h), windows per tile of A1's first pass (cf_count2.hip)
CL_STAGE = 2048               # windows per staging tile of cf_cloud_kernel
CL_COUNT, CL_SMALL, CL_MAX = 512, 1536, 6144      # cloud sizes: counting rank / bitonic in the small set / the 8192-slot set
_TR = bytes.maketrans(b"ACGT", b"0123")


def code_of(kmer):
    """2-bit code of an upper-case ACGT byte string, first base most significant (cfhip.h)."""
    return int(kmer.translate(_TR), 4)


def plain(w):
    return not w.translate(None, b"ACGT")


def codes_of(kmers):
    return np.array([code_of(w) for w in kmers], dtype=np.uint64)


# ------------------------------------------------------------------ the reference, restated
def naive_stage2(reads, units, k, max_nonuniq, lo, hi, min_mult=2, min_n=0, max_n=None, min_d=1, max_d=3, min_cov=1, thr=0.8,
                 kmer_set=None, max_pairs=None):
    """reads: list of bytes; units[r]: list of (start, end) inside read r.  Returns every intermediate of stage 2:
    A1 distance_based_kmer_recruitment.py:39-63 (windows holding a symbol other than upper-case A, C, G, T left out, as
    cf_count_kmers documents), A2 :66-82 with the window [lo, hi], A3 read_kmer_cloud.py:17-40, A4 :43-54, A5 :85-128 and A6
    :131-149 of distance_based_kmer_recruitment.py as the literal nested loops.  kmer_set: clouds of this list of k-mers
    instead of the rare ones.  max_pairs: the distance stage is left out (edges = None) when sum |cloud_i| * |cloud_j| over
    the unit pairs exceeds it."""
    non_unique, all_kmers = Counter(), {}
    pres, multi = Counter(), Counter()
    n_windows = n_plain = n_read_kmers = 0
    for r in reads:
        n_windows += max(0, len(r) - k + 1)
        read_freq = Counter()
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if plain(w):
                read_freq[w] += 1
                n_plain += 1
        n_read_kmers += len(read_freq)
        for w, f in read_freq.items():
            pres[w] += 1
            if f > 1:
                non_unique[w] += 1
                multi[w] += 1
            if non_unique[w] <= max_nonuniq:
                all_kmers[w] = all_kmers.get(w, 0) + 1
            elif w in all_kmers:
                del all_kmers[w]
    table = sorted(pres)
    assert all_kmers == {w: pres[w] for w in table if multi[w] <= max_nonuniq}      # (the loop above has this closed form)
    rare = sorted(w for w, f in all_kmers.items() if lo <= f <= hi)
    kmers = rare if kmer_set is None else list(kmer_set)
    index = {w: i for i, w in enumerate(kmers)}
    clouds = []                                   # per read, per unit: sorted ranks
    for r, us in zip(reads, units):
        mine = []
        for s, e in us:
            row = r[s:e].upper()
            found = set()
            for i in range(len(row) - k + 1):
                w = row[i:i + k]
                if w in index:
                    found.add(w)
            mine.append(sorted(index[w] for w in found))
        clouds.append(mine)
    mult = Counter(x for mine in clouds for c in mine for x in c)
    filtered = [[[x for x in c if mult[x] >= min_mult] for c in mine] for mine in clouds]
    sel = clouds[min_n:max_n]
    est = sum(len(mine[i]) * len(mine[i + d]) for mine in sel for d in range(max(min_d, 1), max_d + 1) for i in range(len(mine) - d))
    edges = unique = E = None
    if max_pairs is None or est <= max_pairs:
        dist_cnt = {d: defaultdict(lambda: defaultdict(int)) for d in range(min_d, max_d + 1)}
        for dist in range(min_d, max_d + 1):
            dt = dist_cnt[dist]
            for mine in sel:
                for i, i_cloud in enumerate(mine[:-dist]):
                    j_cloud = mine[i + dist]
                    for a in i_cloud:
                        row = dt[a]
                        for b in j_cloud:
                            if a != b:
                                row[b] += 1
        cand, all_occ = {}, defaultdict(int)      # all_occ[(a, b)]: the reference's sum over the distances, gathered in one sweep
        for dist, dt in dist_cnt.items():
            for a, row in dt.items():
                for b, freq in row.items():
                    all_occ[(a, b)] += freq
                    if freq >= min_cov:
                        cand[(a, b, dist)] = freq
        E = sum(all_occ.values())
        edges, picked = [], set()
        for (a, b, dist), freq in cand.items():
            if freq / all_occ[(a, b)] >= thr:
                picked.update((a, b))
                edges.append((dist, a, b, freq))
        edges = np.array(sorted(edges), dtype=np.int64).reshape(-1, 4)
        unique = np.array(sorted(picked), dtype=np.int64)

    def csr(cl):
        flat = [c for mine in cl for c in mine]
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in flat], dtype=np.int64)]).astype(np.int64)
        return ptr, np.array([x for c in flat for x in c], dtype=np.int32)

    cloud_ptr, entries = csr(clouds)
    f_ptr, f_entries = csr(filtered)
    return dict(keys=codes_of(table), pres=np.array([pres[w] for w in table], np.uint32), multi=np.array([multi[w] for w in table], np.uint32),
                n_bases=sum(len(r) for r in reads), n_windows=n_windows, n_plain=n_plain, n_read_kmers=n_read_kmers, n_distinct=len(table),
                rare_kmers=rare, kmers=kmers, set_codes=codes_of(kmers), cloud_ptr=cloud_ptr, entries=entries, f_cloud_ptr=f_ptr,
                f_entries=f_entries, sizes=np.diff(cloud_ptr), est_pairs=est, E=E, edges=edges, unique=unique)


def from_arrays(bases, read_off, unit_ptr, unit_start, unit_end):
    """The arrays of Engine.load_arrays -> (reads, units) of naive_stage2."""
    raw = np.asarray(bases, np.uint8).tobytes()
    reads = [raw[int(read_off[r]):int(read_off[r + 1])] for r in range(len(read_off) - 1)]
    units = [[(int(unit_start[u] - read_off[r]), int(unit_end[u] - read_off[r])) for u in range(int(unit_ptr[r]), int(unit_ptr[r + 1]))]
             for r in range(len(reads))]
    return reads, units


def to_arrays(reads, units):
    read_off = np.concatenate([[0], np.cumsum([len(r) for r in reads], dtype=np.int64)]).astype(np.int64)
    unit_ptr = np.concatenate([[0], np.cumsum([len(u) for u in units], dtype=np.int64)]).astype(np.int64)
    us = np.array([read_off[r] + s for r, u in enumerate(units) for s, _ in u], np.int64)
    ue = np.array([read_off[r] + e for r, u in enumerate(units) for _, e in u], np.int64)
    return np.frombuffer(b"".join(reads), np.uint8), read_off, unit_ptr, us, ue


# ------------------------------------------------------------------ the device against it
DIST_PAIRS = 40000      # pair emissions the literal loops of A5 are given; beyond, the distance stage runs on a thinned k-mer set


def naive_of(case, **kw):
    p = dict(min_mult=case.get("min_mult", 2), min_d=case.get("min_d", 1), max_d=case.get("max_d", 3), min_cov=case.get("min_cov", 1),
             thr=case.get("thr", 0.8), max_pairs=DIST_PAIRS)
    p.update(kw)
    return naive_stage2(case["reads"], case["units"], case["k"], case["max_nonuniq"], case["lo"], case["hi"], **p)


def _check_clouds(engine, nv, what):
    n = engine.build_clouds()
    cp, ent = engine.clouds()
    assert n == nv["entries"].size, what
    assert np.array_equal(cp, nv["cloud_ptr"]), f"{what}: cloud_ptr"
    assert np.array_equal(ent, nv["entries"]), f"{what}: entries"


def _check_dist(engine, case, nv, what):
    engine.reset_unique()
    R = len(case["reads"])
    ne = engine.dist_edges(0, R, case.get("min_d", 1), case.get("max_d", 3), case.get("min_cov", 1), case.get("thr", 0.8), 0, 1,
                           edge_cap=nv["edges"].shape[0] + 8)
    assert engine.stats()["n_emissions"] == nv["E"], f"{what}: pair emissions"
    assert ne == nv["edges"].shape[0], f"{what}: number of edges"
    assert np.array_equal(pathcheck.sorted_edges(engine.edges(ne)), nv["edges"]), f"{what}: A5 + A6 edges"
    assert np.array_equal(np.flatnonzero(engine.unique_mask()), nv["unique"]), f"{what}: unique k-mers"


def check_shapes(engine, case, upto="A6", dist=True):
    """A1 -> A2 (upto="A2": no further) -> A3 -> A5/A6 (unless dist is False) -> A4 of one case; the whole table, the counters, the rare set, both cloud CSRs, the edges, the
    emissions and the unique mask.  Where the literal loops of A5 would take more than DIST_PAIRS emissions the distance stage
    runs on every s-th rare k-mer instead (cf_set_kmers, clouds compared again), s from the naive clouds.  Returns the naive
    result."""
    what = case["name"]
    nv = case.get("naive") or naive_of(case)
    case["naive"] = nv
    case["regime"](nv)                                   # from the reference alone, before the device is asked
    engine.load_arrays(*to_arrays(case["reads"], case["units"]))
    k = case["k"]
    engine.count_kmers(k)
    st = engine.stats()
    assert (st["n_bases"], st["n_windows"], st["n_read_kmers"]) == (nv["n_bases"], nv["n_windows"], nv["n_read_kmers"]), what
    keys, pres, multi = engine.table()
    assert np.array_equal(keys, nv["keys"]), f"{what}: A1 keys"
    assert np.array_equal(pres, nv["pres"]), f"{what}: A1 presence counts"
    assert np.array_equal(multi, nv["multi"]), f"{what}: A1 multi-occurrence counts"
    n = engine.select_rare(case["max_nonuniq"], case["lo"], case["hi"])
    assert n == len(nv["rare_kmers"]), f"{what}: size of the rare set"
    assert np.array_equal(engine.kmers(), nv["set_codes"]), f"{what}: A2 rare set"
    assert engine.stats()["n_distinct"] == nv["n_distinct"], what
    if upto == "A2":
        return nv
    if case.get("refused"):
        try:
            engine.build_clouds()
        except DeviceError as e:
            assert "(-34)" in str(e) and str(CL_MAX) in str(e), str(e)
            return nv
        raise AssertionError(f"{what}: cf_build_clouds accepted a cloud of {int(nv['sizes'].max())} entries")
    _check_clouds(engine, nv, what)
    if dist and nv["edges"] is not None:
        _check_dist(engine, case, nv, what)
    assert engine.filter_clouds(case.get("min_mult", 2)) == nv["f_entries"].size, what
    cp, ent = engine.clouds()
    assert np.array_equal(cp, nv["f_cloud_ptr"]) and np.array_equal(ent, nv["f_entries"]), f"{what}: A4 filtered clouds"
    if dist and nv["edges"] is None:
        s = int(math.ceil(math.sqrt(nv["est_pairs"] / DIST_PAIRS)))      # (clouds shrink by about s, their pairs by s * s)
        thin = case.get("thin") or naive_of(case, kmer_set=nv["rare_kmers"][::s], max_pairs=4 * DIST_PAIRS)
        case["thin"] = thin
        assert thin["edges"] is not None and len(thin["kmers"]) > 0, what
        engine.set_kmers(thin["set_codes"], k)
        _check_clouds(engine, thin, what + " (thinned set)")
        _check_dist(engine, case, thin, what + " (thinned set)")
    return nv


def check_occurrences(engine, reads, k, ns="all"):
    """cf_count_occurrences + cf_top_kmers against a Counter over every window: the table, and the n k-mers with the largest
    (count, k-mer), descending, for n below, at and above the number of distinct k-mers and with a tie at the cut (ns = "few": one n
    with a tie at the cut, D and D + 1; "one": the tie alone — the emulator takes half a second per request)."""
    cnt = Counter(r[i:i + k] for r in reads for i in range(len(r) - k + 1))
    assert all(plain(w) for w in cnt)
    table = sorted(cnt)
    engine.load_arrays(*to_arrays(reads, [[] for _ in reads]))
    engine.count_occurrences(k)
    keys, lo, hi = engine.table()
    assert np.array_equal(keys, codes_of(table)), "occurrence table: keys"
    assert np.array_equal(lo.astype(np.int64) | (hi.astype(np.int64) << 32), np.array([cnt[w] for w in table], np.int64)), "occurrence counts"
    order = sorted(cnt.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    D = len(order)
    ties = [n for n in range(1, D) if order[n - 1][1] == order[n][1]]
    assert ties, "no two k-mers of equal count: the case lost its tie at the cut"
    tie = ties[len(ties) // 2]
    for n in {"one": [tie], "few": [tie, D, D + 1], "all": sorted({0, 1, ties[0], tie, ties[-1], D - 1, D, D + 1, 10 ** 9})}[ns]:
        tk, tc = engine.top_kmers(n)
        want = order[:n]
        assert np.array_equal(tk, codes_of([w for w, _ in want])), f"top {n} of {D}: k-mers"
        assert np.array_equal(tc.astype(np.int64), np.array([c for _, c in want], np.int64)), f"top {n} of {D}: counts"
    return D


# ------------------------------------------------------------------ builders
def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def cloud_regime(n):
    return "count" if n <= CL_COUNT else "bitonic" if n <= CL_SMALL else "retry" if n <= CL_MAX else "refused"


def _one_read_case(name, seed, unit_windows, k=19):
    """One random read; units of length 10 (< k), k, k - 1 and one unit of exactly n windows for every n of unit_windows."""
    rng = np.random.default_rng(seed)
    units, pos = [(0, 10), (10, 10 + k), (10 + k, 9 + 2 * k)], 12 + 2 * k
    for n in unit_windows:
        units.append((pos, pos + n + k - 1))
        pos += n + k - 1 + 3
    read = rand_seq(rng, pos + 7)
    want = [0, 1, 0] + list(unit_windows)

    def regime(nv):
        assert nv["n_distinct"] == nv["n_windows"] == len(read) - k + 1, "the read's k-mers are not all different"
        assert nv["sizes"].tolist() == want, (nv["sizes"].tolist(), want)
    return dict(name=name, reads=[read], units=[units], k=k, max_nonuniq=3, lo=1, hi=1, regime=regime, refused=max(unit_windows) > CL_MAX)


CLOUD_SIZES = (400, 512, 513, 1536, 1537, 2100, 5000, 6144)


def cloud_size_case(n):
    """Family 1: the four regimes of cf_cloud_kernel by the number of distinct set k-mers of one unit."""
    c = _one_read_case(f"cloud of {n} ({cloud_regime(n)})", 1000 + n, [n])
    inner = c["regime"]
    want = {400: "count", 512: "count", 513: "bitonic", 1536: "bitonic", 1537: "retry", 2100: "retry", 5000: "retry", 6144: "retry", 6145: "refused"}[n]

    def regime(nv):
        inner(nv)
        assert cloud_regime(int(nv["sizes"].max())) == want and int(nv["sizes"].max()) == n
    c["regime"] = regime
    return c


def cloud_mixed_case():
    """A small unit and a 5000-entry unit in one launch (the retry repeats units that had succeeded), in two reads."""
    a = _one_read_case("", 77, [300, 5000])
    b = _one_read_case("", 78, [1, 700, 1600])
    want = [0, 1, 0, 300, 5000, 0, 1, 0, 1, 700, 1600]

    def regime(nv):
        assert nv["sizes"].tolist() == want and cloud_regime(int(nv["sizes"].max())) == "retry"
    return dict(name="small and 5000-entry units in one launch", reads=a["reads"] + b["reads"], units=a["units"] + b["units"], k=19,
                max_nonuniq=3, lo=1, hi=1, regime=regime)


def cloud_staging_case():
    """Units of 2048, 2049, 4096 and 4097 windows: at and one past the staging tile of 2048 windows, once and twice."""
    c = _one_read_case("staging-tile borders", 79, [CL_STAGE, CL_STAGE + 1, 2 * CL_STAGE, 2 * CL_STAGE + 1])
    c["name"] = "units of 2048, 2049, 4096, 4097 windows"
    return c


A1_KS = (1, 2, 3, 4, 5, 8, 13, 16, 17, 24, 27, 30, 31)
_BAD = (ord("N"), ord("c"), 0x80, ord("t"), 0xC7, ord("n"))


def a1_lengths(k):
    return [0, 1, k - 1, k, k + 1, TILE + k - 2, TILE + k - 1, TILE + k, 2 * TILE + k + 1]


def a1_case(k, e, symbols):
    """Family 2.  Reads of the lengths a1_lengths(k), each after a short read of 1 .. 4 bases that puts the j-th of them at the
    offset (e + j) mod 4 of the base array (e = 0 .. 3: every read at every offset in turn); a last read that ends the array at
    n_bases = e (mod 4).  symbols: N, lower-case letters and bytes >= 0x80, each alone among plain bases: in every byte lane of
    a word (bases 0, 41, 82, 123 of the four long reads), in the last base of a read, under the last window of a tile only
    (base 4095), under the first window of a tile only (base 4096 + k - 1 of the read of 4097 windows, 8192 + k - 1 of the
    longest), inside a tile, and in the last base of the array.  Reads of up to 4096 + k bases are one unit, the longest one is
    cut into units of 3000 bases."""
    rng = np.random.default_rng(100 * k + 10 * e + symbols)
    reads, starts, pos = [], [], 0
    lens = a1_lengths(k)
    for j, L in enumerate(lens):
        pad = ((e + j) - pos - 1) % 4 + 1               # 1 .. 4 bases
        reads.append(rand_seq(rng, pad)); pos += pad
        starts.append(pos)
        reads.append(rand_seq(rng, L)); pos += L
    tail = k + 1 + (e - (pos + k + 1)) % 4
    reads.append(rand_seq(rng, tail))
    long_reads = [2 * j + 1 for j in range(len(lens) - 4, len(lens))]      # 4095, 4096, 4097 and 8194 windows
    if symbols:
        border = {0: lambda L: [L - 1], 1: lambda L: [TILE - 1], 2: lambda L: [TILE + k - 1], 3: lambda L: [TILE - 1, TILE + 1000, 2 * TILE + k - 1]}
        n = 0
        for q, i in enumerate(long_reads):
            r = bytearray(reads[i])
            for p in [0, 41, 82, 123] + border[q](len(r)):
                r[p] = _BAD[n % len(_BAD)]; n += 1
            reads[i] = bytes(r)
        r = bytearray(reads[-1]); r[-1] = _BAD[e]; reads[-1] = bytes(r)
    units = [[(s, min(s + 3000, len(r))) for s in range(0, len(r), 3000)] if len(r) > TILE + k else [(0, len(r))] for r in reads]
    R = len(reads)

    def regime(nv):
        assert nv["n_bases"] % 4 == e
        assert [s % 4 for s in starts] == [(e + j) % 4 for j in range(len(lens))]
        wins = [max(0, len(reads[2 * j + 1]) - k + 1) for j in range(len(lens))]
        assert wins[0] == 0 and wins[2] == 0 and wins[3:] == [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2], wins
        assert (nv["n_plain"] < nv["n_windows"]) == bool(symbols)
        if symbols:
            r = reads[long_reads[2]]
            assert plain(r[TILE - 1:TILE - 1 + k]) and not plain(r[TILE:TILE + k])             # tile 0's last window stands, tile 1's only one falls
            r = reads[long_reads[3]]
            assert not plain(r[TILE - 1:TILE - 1 + k]) and plain(r[TILE:TILE + k])             # ... and the other way round
            assert plain(r[2 * TILE - 1:2 * TILE - 1 + k]) and not plain(r[2 * TILE:2 * TILE + k])
            assert not plain(reads[-1][-k:]) and not plain(reads[long_reads[0]][-k:])
        top = int(nv["sizes"].max())
        if k >= 8:        # (4^k far beyond the read lengths: a unit of 4096 + 1 windows is a cloud of the 8192-slot set)
            assert CL_SMALL < top <= CL_MAX, top
        elif k == 5:
            assert CL_COUNT < top <= CL_SMALL, top
        else:
            assert 0 < top <= CL_COUNT
    return dict(name=f"A1 k={k} offset {e}{' with other symbols' if symbols else ''}", reads=reads, units=units, k=k, max_nonuniq=R, lo=1,
                hi=R, regime=regime, max_d=2)


def repeats_case(R, k, max_nonuniq):
    """Family 3: R reads of ~6000 bases, one 600-base stretch twice in every read (shared between the reads); units
    (0, 2055), (2055, 4110), (4110, end); rare window [1, R]."""
    rng = np.random.default_rng(7000 + 10 * R + k)
    stretch = rand_seq(rng, 600)
    reads = []
    for r in range(R):
        a, b, c = rand_seq(rng, 700 + 40 * r), rand_seq(rng, 2600 - 13 * r), rand_seq(rng, 1500 + r)
        reads.append(a + stretch + b + stretch + c)
    units = [[(0, 2055), (2055, 4110), (4110, len(r))] for r in reads]

    def regime(nv):
        assert int(nv["multi"].max()) == R and int(nv["pres"].max()) == R
        cut = int((nv["multi"] > max_nonuniq).sum())
        assert (cut > 0) == (R > max_nonuniq) and (cut >= 600 - k + 1 or k == 4 or not cut), (cut, R, max_nonuniq)
        if k >= 11:
            assert len(nv["rare_kmers"]) > 1000 * R
    return dict(name=f"{R} reads with a repeat, k={k}, max_nonuniq={max_nonuniq}", reads=reads, units=units, k=k, max_nonuniq=max_nonuniq,
                lo=1, hi=R, regime=regime, max_d=2, thr=0.5)


# (reads, units per read, cloud sizes lo .. hi, empty every, k-mers, min_d, max_d, min_cov, threshold)
DENSE = {
    "dense_2x5": (2, 5, 300, 1200, 0, 3000, 1, 4, 2, 0.5),
    "dense_3x4_holes": (3, 4, 0, 900, 3, 1500, 0, 3, 1, 0.8),
    "dense_2x6_flat": (2, 6, 700, 701, 0, 800, 2, 9, 2, 0.3),
    "one_unit": (1, 1, 600, 900, 0, 1000, 1, 4, 1, 0.8),
    "tiny_set": (4, 3, 1, 2, 0, 5, 1, 1, 1, 1.0),
}
DENSE_SMALL = ("one_unit", "tiny_set")


def dense_clouds(name):
    n_reads, per, lo, hi, holes, n_kmers = DENSE[name][:6]
    rng = np.random.default_rng(sum(name.encode()))
    ent, cp = [], [0]
    for u in range(n_reads * per):
        size = 0 if holes and u % holes == 2 else int(rng.integers(lo, hi + 1))
        ent.append(np.sort(rng.choice(n_kmers, size, replace=False)).astype(np.int32))
        cp.append(cp[-1] + size)
    return np.arange(n_reads + 1, dtype=np.int64) * per, np.array(cp, np.int64), np.concatenate(ent), n_kmers


def check_dense(engine, name):
    """Family 4: the distance stage on dense hand-made clouds (pathcheck.check_clouds: the numpy oracle's histogram and filter).
    The regime is asserted on the clouds themselves and on the oracle's edges.  Returns the oracle's edges."""
    n_reads, per, lo, hi, holes, n_kmers, min_d, max_d, min_cov, thr = DENSE[name]
    unit_ptr, cloud_ptr, entries, n_kmers = dense_clouds(name)
    sizes = np.diff(cloud_ptr)
    assert sizes.size == n_reads * per and int(sizes.max()) <= hi and int(sizes[sizes > 0].min()) >= max(lo, 1)
    if holes:
        assert (sizes[2::holes] == 0).all() and int((sizes == 0).sum()) >= sizes.size // holes
    if name.startswith("dense"):
        assert int(sizes.max()) > 2 * 256 and sizes.sum() > 2 * n_kmers      # several 256-entry items from one partner unit; every k-mer's (b, d) slots fill
    edges = pathcheck.check_clouds(engine, unit_ptr, cloud_ptr, entries, n_kmers, min_d, max_d, min_cov, thr)
    if per > 1:
        assert edges.shape[0] > (100000 if name.startswith("dense") else 0), edges.shape
    else:
        assert edges.shape[0] == 0
    return edges


# ------------------------------------------------------------------ the generic radix sort and scan (cf_prims.hip)
def stable_sorted(keys, bits):
    sorted_bits = (bits + 7) // 8 * 8
    low = keys & np.uint64((1 << sorted_bits) - 1) if sorted_bits < 64 else keys
    return keys[np.argsort(low, kind="stable")]


def radix_across_tile_boundaries(engine, n):
    rng = np.random.default_rng(n)
    k = rng.integers(0, 2 ** 24, n, dtype=np.uint64)
    assert np.array_equal(engine.selftest_sort(k, 24), np.sort(k))


def radix_stable_on_odd_widths(engine, bits):
    rng = np.random.default_rng(bits)
    n = 2 * TILE + 999
    sorted_bits = (bits + 7) // 8 * 8
    key = rng.integers(0, 2 ** bits, n, dtype=np.uint64)
    payload = np.arange(n, dtype=np.uint64) % np.uint64(1 << (62 - sorted_bits))     # ascending: the input order
    k = key | (payload << np.uint64(sorted_bits))
    assert np.array_equal(engine.selftest_sort(k, bits), stable_sorted(k, bits))


def radix_skewed_digits(engine):
    rng = np.random.default_rng(5)
    n = 5 * TILE + 3
    key = np.where(rng.random(n) < 0.9, 7, rng.integers(0, 1 << 16, n)).astype(np.uint64)      # one digit fills whole tiles
    k = key | (np.arange(n, dtype=np.uint64) << np.uint64(16))
    assert np.array_equal(engine.selftest_sort(k, 16), stable_sorted(k, 16))


def radix_grid_strides(engine, tiles):
    """tiles * 4096 + 5 keys on a grid of at most 8 workgroups per CU: random 64-bit keys, and 13-bit keys under the input index
    as a payload above bit 16 (two digits sorted: the payload must keep its order inside every key)."""
    rng = np.random.default_rng(9)
    n = tiles * TILE + 5
    k = rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64)
    assert np.array_equal(engine.selftest_sort(k, 64), np.sort(k))
    key = rng.integers(0, 2 ** 13, n, dtype=np.uint64)
    k = key | (np.arange(n, dtype=np.uint64) << np.uint64(16))
    want = k[np.argsort(k & np.uint64(0xFFFF), kind="stable")]
    assert np.array_equal(engine.selftest_sort(k, 13), want)


def scan_of_wide_values(engine, n):
    """Exclusive scan of values in [2^39, 2^40): every partial sum is far beyond 32 bits."""
    v = np.random.default_rng(n).integers(2 ** 39, 2 ** 40, n, dtype=np.int64)
    assert np.array_equal(engine.selftest_scan(v), np.concatenate([[0], np.cumsum(v)]))

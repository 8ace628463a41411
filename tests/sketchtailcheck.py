"""The distance stage with the sketch sweep cut at d*(a) (knob dist_sketch_tail) on hand-built reads, against the plain
restatement shapecheck.naive_stage2.

A cloud row is a set, so cnt(a, b, d) <= P_d(a), the number of postings of a whose partner range has a unit at distance d; d*(a) is
the largest d with P_d(a) >= min_cov, and the sketch sweep leaves out the items (256 consecutive partner entries of a posting) whose
first entry lies beyond d*.  The reads here are made of k-mers chosen one by one: a unit is its k-mers' texts joined by "N", so its
cloud is exactly that set, a first k-mer sits in the units it was put into and nowhere else, and the sizes of the units between a
posting and a planted partner put the planted partner at the start of an item where the case needs it there.  Every case runs with
the knob at 1 and at 0 and compares n_emissions, n_edges, the edges as a sorted list and the unique mask with the naive result; what a
case was built for (an edge that must be there, a pair that must not) is asserted on the naive result alone, before the device runs.
Used by test_emu_dist_sketch_tail.py (host emulator) and test_gpu_dist_sketch_tail.py (MI355X)."""
import numpy as np

import shapecheck

K = 13
ITEM = 256      # DIST_ITEM of cf_dist.hip


def _texts(n, seed):
    """n different k-mers, ascending: the rank of a k-mer among those a read set uses follows its number here."""
    rng = np.random.default_rng(seed)
    codes = np.unique(rng.integers(0, 4 ** K, 2 * n + 16))[:n]
    assert codes.size == n
    return [bytes(b"ACGT"[(int(c) >> (2 * (K - 1 - i))) & 3] for i in range(K)) for c in codes]


def reads_of(layout, n_ids, seed):
    """layout[r][u] = the k-mer numbers of unit u of read r -> (reads, units) of naive_stage2 and the texts by number."""
    texts = _texts(n_ids, seed)
    reads, units = [], []
    for rd in layout:
        buf, us, pos = [], [], 0
        for unit in rd:
            s = b"N".join(texts[x] for x in unit)
            us.append((pos, pos + len(s)))
            buf.append(s + b"N")
            pos += len(s) + 1
        reads.append(b"".join(buf))
        units.append(us)
    return reads, units, texts


def _fill(rng, unit, size, pool):
    """unit (planted numbers) filled up to `size` numbers with different ones of the pool."""
    assert len(unit) <= size
    return sorted(set(unit) | set(rng.choice(pool, size - len(unit), replace=False).tolist()))


# ------------------------------------------------------------------ the read sets
A, Z, ZB, B1, B2, B3, B4 = 0, 1, 2, 3, 4, 5, 6
CORE_TAILS = (27, 9, 8, 7)      # units behind the posting of A in the four reads: all different; the min_cov-th largest (min_cov 4) is 7 = d*(A)
CORE_SIZES = (43, 43, 43, 43, 42, 42)      # the units at the distances 1 .. 6 hold 256 entries: the unit at distance 7 begins an item


def core_layout():
    """A in unit 0 of four reads with 27, 9, 8 and 7 units behind it: d*(A) = 7 at min_cov 4, min_d 1.  The units at the distances
    1 .. 6 hold exactly 256 entries in every read, so the unit at distance 7 starts the second item of every posting, and that item
    runs on into distance 8: it straddles the boundary.  In the long read 19 more units (more than three whole items) lie beyond it.
      B1  at distance 7 in all four reads: cnt 4 = min_cov exactly at d*, total 4 -> selected
      B2  at distance 8 (d* + 1) in the three reads that have one: cnt 3 -> not selected
      B3  at distance 7 four times and at distance 9 twice: 5 * 4 < 4 * 6 -> not selected; without the two occurrences beyond d* in the
          filter's total it would be (5 * 4 >= 4 * 4)
      B4  at distance 7 four times and at distance 15 once: 5 * 4 >= 4 * 5 -> selected with the total 5
      Z   in unit 0 of three reads and in the last unit of the long one: three postings with a partner unit, fewer than min_cov
          (nA = 0); ZB at distance 3 behind each of the three: cnt 3 -> not selected."""
    rng = np.random.default_rng(11)
    pool = np.arange(100, 500)
    plants = {7: [(B1, (0, 1, 2, 3)), (B3, (0, 1, 2, 3)), (B4, (0, 1, 2, 3))], 8: [(B2, (0, 1, 2))], 9: [(B3, (0, 1))], 15: [(B4, (0,))], 3: [(ZB, (1, 2, 3))]}
    layout = []
    for r, t in enumerate(CORE_TAILS):
        rd = []
        for u in range(t + 1):
            unit = [x for x, rs in plants.get(u, []) if r in rs]
            if u == 0:
                unit += [A] + ([Z] if r else [])
            if u == t and r == 0:
                unit.append(Z)
            size = 6 if u == 0 else CORE_SIZES[u - 1] if u <= len(CORE_SIZES) else 43
            rd.append(_fill(rng, unit, size, pool))
        layout.append(rd)
    return layout, 500


POSTINGS = (16, 17, 64, 65)


def postings_layout():
    """First k-mers P_n with n = 16, 17, 64 and 65 postings (one, two and four 16-lane rounds of the builder's selection, and the
    list that is too long for it).  Three postings of each have 8 partner units (unit 1 of three reads of 10 units whose units at the
    distances 1 .. 4 hold 256 entries), n - 4 have one (unit 0 of reads of two units) and the LAST posting of the list, in the last read,
    has 5: d*(P_n) = 5 at min_cov 4, decided by the posting the selection sees last.  Q_n at distance 5 behind the four long postings:
    cnt 4 at d* -> selected; in the three long reads it opens the second item."""
    rng = np.random.default_rng(12)
    pool = np.arange(100, 400)
    P = {n: 2 * i for i, n in enumerate(POSTINGS)}
    Q = {n: 2 * i + 1 for i, n in enumerate(POSTINGS)}
    layout = []
    for r in range(3):
        sizes = [10, 12, 64, 64, 64, 64, 64, 30, 30, 30]
        layout.append([_fill(rng, list(P.values()) if u == 1 else list(Q.values()) if u == 6 else [], sizes[u], pool) for u in range(10)])
    for s in range(max(POSTINGS) - 4):
        layout.append([_fill(rng, [P[n] for n in POSTINGS if s < n - 4], 8, pool), _fill(rng, [], 6, pool)])
    sizes = [8, 8, 10, 10, 10, 10, 12]
    layout.append([_fill(rng, list(P.values()) if u == 1 else list(Q.values()) if u == 6 else [], sizes[u], pool) for u in range(7)])
    return layout, 400, P, Q


def _ranks(nv, texts, ids):
    index = {w: i for i, w in enumerate(nv["kmers"])}
    return [index[texts[x]] for x in ids]


def _edge_map(nv):
    return {(int(a), int(b)): (int(d), int(c)) for d, a, b, c in nv["edges"]}


_cases = {}


def case(name, min_d=1, max_d=150, min_cov=4):
    """The case (cached: the naive result is computed once per read set and parameters and shared by every run of it)."""
    key = (name, min_d, max_d, min_cov)
    if key in _cases:
        return _cases[key]
    if name == "core":
        layout, n_ids = core_layout()
        reads, units, texts = reads_of(layout, n_ids, 21)
    else:
        layout, n_ids, P, Q = postings_layout()
        reads, units, texts = reads_of(layout, n_ids, 22)
    R = len(reads)
    c = dict(name=f"{name} min_d={min_d} max_d={max_d} min_cov={min_cov}", reads=reads, units=units, k=K, max_nonuniq=R, lo=1, hi=R,
             min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv = shapecheck.naive_stage2(reads, units, K, R, 1, R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    c["naive"] = nv
    got = _edge_map(nv)
    if name == "core":
        a, z, zb, b1, b2, b3, b4 = _ranks(nv, texts, [A, Z, ZB, B1, B2, B3, B4])
        sizes = nv["sizes"].tolist()
        at = np.concatenate([[0], np.cumsum([len(u) for u in units])])
        for r in range(R):      # 256 entries between the posting and distance 7, and item 2 runs on into distance 8
            assert sum(sizes[at[r] + 1:at[r] + 7]) == ITEM and 0 < sizes[at[r] + 7] < ITEM, sizes[at[r]:at[r] + 9]
        assert sum(sizes[at[0] + 9:at[1]]) > 3 * ITEM      # the long read: whole items beyond d*
        if (min_d, min_cov) == (1, 4) and max_d >= 15:
            assert got.get((a, b1)) == (7, 4) and got.get((a, b4)) == (7, 4), "the pairs that reach min_cov exactly at d*"
            assert (a, b2) not in got and (a, b3) not in got, "one posting short at d* + 1 / the occurrences beyond d* in the total"
            assert not [1 for (x, _) in got if x == z], "Z has three postings with a partner unit"
        if min_cov <= 3 and max_d >= 8:
            assert got.get((a, b2)) == (8, 3)
    else:
        for n in POSTINGS:
            p, q = _ranks(nv, texts, [P[n], Q[n]])
            assert int((nv["entries"] == p).sum()) == n, "postings of P_n"
            if min_cov == 4 and min_d <= 5 <= max_d:
                assert got.get((p, q)) == (5, 4), n
    _cases[key] = c
    return c


# ------------------------------------------------------------------ the device against it
def run(engine, c, knobs=None):
    """A1 .. A3 once, then the distance stage under `knobs` with dist_sketch_tail 1 and 0."""
    nv, what = c["naive"], c["name"]
    engine.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    engine.count_kmers(c["k"])
    assert engine.select_rare(c["max_nonuniq"], c["lo"], c["hi"]) == len(nv["rare_kmers"])
    assert np.array_equal(engine.kmers(), nv["set_codes"])
    shapecheck._check_clouds(engine, nv, what)
    knobs = dict(knobs or {})
    for tail in (1, 0):
        with engine.knobs(**knobs, dist_sketch_tail=tail):
            shapecheck._check_dist(engine, c, nv, f"{what} {knobs} dist_sketch_tail={tail}")
    return engine.stats()


# the other table layouts, a table that splits, byte counters, one workgroup per CU
LAYOUTS = {
    "wide": dict(dist_wide=1),
    "regions26": dict(dist_regions=2),
    "region_bytes": dict(dist_regions=2, dist_region_bytes=1),
    "sketch_bytes": dict(dist_sketch_bits=8),
    "one_workgroup": dict(dist_wgs=1),
}
PARAMS = [dict(min_cov=1), dict(min_cov=2), dict(min_cov=4), dict(max_d=12), dict(max_d=5), dict(min_d=2), dict(min_d=2, max_d=12, min_cov=2)]


def repeated_rank_clouds():
    """Clouds for cf_set_clouds in which one unit holds a rank twice: the row is not a set, cnt(a, b, d) may exceed P_d(a), and the
    builder must declare every item useful.  Five reads of 8 units; first k-mer 0 in unit 0 of reads 0 .. 2 only (three postings, fewer
    than min_cov 4: nA would be 0), and rank 1 TWICE in unit 2 of reads 0 and 1: cnt(0, 1, 2) = 4 -> an edge the cut would lose."""
    rng = np.random.default_rng(13)
    n_kmers, per = 120, 8
    ent, cp = [], [0]
    for r in range(5):
        for u in range(per):
            row = np.sort(rng.choice(np.arange(2, n_kmers), 40, replace=False)).tolist()
            if u == 0 and r < 3:
                row = [0] + row
            if u == 2 and r < 2:
                row = [1, 1] + row
            ent += row
            cp.append(len(ent))
    return np.arange(6, dtype=np.int64) * per, np.array(cp, np.int64), np.array(ent, np.int32), n_kmers


def run_repeated_rank(engine):
    import pathcheck
    unit_ptr, cloud_ptr, entries, n_kmers = repeated_rank_clouds()
    for tail in (1, 0):
        with engine.knobs(dist_sketch_tail=tail):
            edges = pathcheck.check_clouds(engine, unit_ptr, cloud_ptr, entries, n_kmers, 1, 150, 4, 0.8)
        assert [2, 0, 1, 4] in edges.tolist(), "the case lost its edge"


def run_exchange(lib, rendezvous, knobs=None, n_units=6, n_reads=200):
    """A few hundred generator reads through the exchange path of one rank (bucketing, all-to-all, all-gathers, the gathered view of the
    clouds) with the knob at 1, against the plain-C oracle."""
    from centroflye_amd import _host
    from centroflye_amd.sharded import ShardedRecruiter
    from oracle import cport
    pk = _host.synth(seed=17, n_units=n_units, n_reads=n_reads, var_len=8)
    up, us, ue, _ = pk.units(1)
    c, a = cport.stage2(pk.bases, pk.read_off, up, us, ue, 19, 3, 10, 32, 0, 2 ** 62, 1, 150, 4, 0.8, want_arrays=True)
    assert c["n_edges"] > 1000
    sr = ShardedRecruiter(0, lib=lib, rank=0, world=1, rendezvous=rendezvous, force_exchange=True)
    try:
        for name, value in (knobs or {}).items():
            sr.engine.set_param(name, value)
        sr.engine.set_param("dist_sketch_tail", 1)
        sr.load(pk, 1)
        out = sr.run(k=19, max_nonuniq=3, lo=10, hi=32, min_d=1, max_d=150, min_cov=4, rel_threshold=0.8, edge_cap=c["n_edges"] + 8)
        assert (out["n_edges"], out["n_emissions"]) == (c["n_edges"], c["n_emissions"])
        import pathcheck
        assert np.array_equal(pathcheck.sorted_edges(sr.engine.edges(out["local_edges"])), pathcheck.sorted_edges(a["edges"]))
        assert np.array_equal(sr.unique_mask, a["unique"])
    finally:
        sr.close()

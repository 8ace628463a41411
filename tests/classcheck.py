"""The distance stage with first k-mers of equal posting lists swept once (knob dist_classes) on hand-built reads, against
the plain restatement shapecheck.naive_stage2.

cnt(a, b, d) depends on the first k-mer a only through its posting list — the units whose cloud holds a.  The library sorts the first
k-mers of a launch so that equal lists stand next to each other, sweeps one k-mer per class and writes, from the one table, the rows of
every member: the same slots and totals, `b != a_j` and the first column its own.  The reads here are made of k-mers chosen one by one
(sketchtailcheck.reads_of: a unit is its k-mers' texts joined by "N"), so a k-mer's posting list is exactly the units it was put into.
Every case first proves FROM NUMPY ALONE (posting lists off the naive clouds, grouped by equality) which classes it contains and what
the naive result must show for them; then the device runs with the knob at 1 and at 0 and n_emissions, n_edges, the edges as a sorted
list and the unique mask are compared with the naive result.
Used by test_emu_dist_classes.py (host emulator) and test_gpu_dist_classes.py (MI355X)."""
import numpy as np

import pathcheck
import shapecheck
import sketchtailcheck as stc

CLASS_CAP = 255      # DIST_CLASS_CAP of cf_dist.hip: members of one class; a longer run of equal lists starts a new class
N_READS = 4          # every planted k-mer stands in all four reads unless the case says otherwise: counts reach min_cov 4 exactly

# ------------------------------------------------------------------ the read sets
# numbers of the planted k-mers (their ranks follow their numbers: sketchtailcheck._texts)
C2 = (0, 1)             # class of 2: unit 0 and unit 4 of every read
C3 = (2, 3, 4)          # class of 3: unit 0 and unit 3 of every read
M = (5, 6)              # class of 2 whose units lie 2 apart in ONE read (units 0 and 2): cnt(M0, M1, 2) = cnt(M0, M0, 2) = 4 — each member is a
                        # selected partner of the other, and the slot b == M0 that M0 must leave out is one that M1 must keep
S = 7                   # singleton in the units 0 and 3 of four reads of their own (filler around it): its slot (b == S, d 3, cnt 4, total 4) is
                        # dominant and is its ONLY slot that reaches min_cov 4 — S has no edge as a first k-mer, and nobody selects it
D1, D2 = 8, 9           # D1: unit 0 of every read; D2: unit 0 of the reads 0 .. 2 and unit 1 of read 3 — same first unit, same length, last unit differs
X = 10                  # C2's list and one posting more (unit 5 of read 3, the last of the list)
P = 11                  # the partner: unit 1 of every read, distance 1 behind unit 0
Q = 12                  # a second partner: unit 6 of the reads 0 .. 2 only (cnt 3 from unit 0)
N_PLANTED = 13
UNITS = 7


def core_layout(fill=5, pool=(20, 120), seed=31):
    rng = np.random.default_rng(seed)
    pool = np.arange(*pool)
    layout = []
    for r in range(N_READS):
        rd = []
        for u in range(UNITS):
            unit = []
            if u == 0:
                unit += list(C2) + list(C3) + list(M) + [D1, X] + ([D2] if r < 3 else [])
            if u == 1:
                unit += [P] + ([D2] if r == 3 else [])
            if u == 2:
                unit += list(M)
            if u == 3:
                unit += list(C3)
            if u == 4:
                unit += list(C2) + [X]
            if u == 5 and r == 3:
                unit += [X]
            if u == 6 and r < 3:
                unit += [Q]
            rd.append(stc._fill(rng, unit, len(unit) + fill, pool))
        layout.append(rd)
    for r in range(N_READS):      # the reads of S
        layout.append([stc._fill(rng, [S] if u in (0, 3) else [], 3, pool) for u in range(4)])
    return layout, int(pool[-1]) + 1


BIG = tuple(range(CLASS_CAP + 1))      # cap + 1 k-mers with one list: a class of 255 and a class of 1
BIG_P = CLASS_CAP + 1
BIG_T = (CLASS_CAP + 2, CLASS_CAP + 3)      # a class of 2 one unit in front of them: 256 and more partners with cnt 4 at distance 1 — its table splits when the slots are few


def big_layout():
    """256 k-mers in unit 1 of every read (one posting list: a run longer than the member cap), their partner in unit 2, a class of 2 in
    unit 0 and a unit of filler at the end."""
    rng = np.random.default_rng(32)
    pool = np.arange(300, 340)
    layout = []
    for r in range(N_READS):
        layout.append([stc._fill(rng, list(BIG_T), 4, pool), stc._fill(rng, list(BIG), len(BIG) + 2, pool), stc._fill(rng, [BIG_P], 4, pool), stc._fill(rng, [], 3, pool)])
    return layout, 340


def wide_rows_layout():
    """Many selected rows per member: a class of 3 in unit 0 and 40 partners in unit 1 of every read (cnt 4 each) — with a small edge
    chunk the rows of one member cross chunks, with a small stage the late rows take the marked-slot sweep, and the marks of one
    member must be gone before the next one's sweep."""
    rng = np.random.default_rng(33)
    pool = np.arange(100, 160)
    partners = list(range(3, 43))
    layout = []
    for r in range(N_READS):
        layout.append([stc._fill(rng, [0, 1, 2], 5, pool), stc._fill(rng, partners, len(partners) + 3, pool), stc._fill(rng, [], 3, pool)])
    return layout, 160


# ------------------------------------------------------------------ what numpy says about a case
def posting_lists(nv):
    """rank -> tuple of the units whose cloud holds it (ascending), off the naive clouds."""
    cp, ent = nv["cloud_ptr"], nv["entries"]
    unit_of = np.repeat(np.arange(cp.size - 1), np.diff(cp))
    lists = {}
    for x, u in zip(ent.tolist(), unit_of.tolist()):
        lists.setdefault(x, []).append(u)
    return {x: tuple(us) for x, us in lists.items()}


def classes_of(nv, part=0, n_parts=1):
    """The classes of equal posting lists among the first k-mers of one partition: list of rank tuples."""
    groups = {}
    for x, us in posting_lists(nv).items():
        if x % n_parts == part:
            groups.setdefault(us, []).append(x)
    return [tuple(sorted(g)) for g in groups.values()]


def capped_classes(nv, part=0, n_parts=1):
    """Fewest classes the library can form (every run cut at the member cap), and the first k-mers they hold."""
    cl = classes_of(nv, part, n_parts)
    return sum(-(-len(g) // CLASS_CAP) for g in cl), sum(len(g) for g in cl)


def _edge_set(nv):
    return {(int(d), int(a), int(b), int(c)) for d, a, b, c in nv["edges"]}


def _rows_of(nv, a):
    return {(int(d), int(b), int(c)) for d, x, b, c in nv["edges"] if x == a}


_cases = {}


def case(name, min_d=1, max_d=150, min_cov=4):
    key = (name, min_d, max_d, min_cov)
    if key in _cases:
        return _cases[key]
    layout, n_ids = {"core": core_layout, "big": big_layout, "rows": wide_rows_layout}[name]()
    reads, units, texts = stc.reads_of(layout, n_ids, 41)
    R = len(reads)
    c = dict(name=f"classes:{name} min_d={min_d} max_d={max_d} min_cov={min_cov}", reads=reads, units=units, k=stc.K, max_nonuniq=R, lo=1, hi=R,
             min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv = shapecheck.naive_stage2(reads, units, stc.K, R, 1, R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    c["naive"] = nv
    cl = set(classes_of(nv))
    lists = posting_lists(nv)
    rk = lambda ids: tuple(stc._ranks(nv, texts, list(ids)))
    if name == "core":
        c2, c3, m = rk(C2), rk(C3), rk(M)
        s, d1, d2, x, p, q = rk([S, D1, D2, X, P, Q])
        # the classes, from the posting lists alone
        assert c2 in cl and c3 in cl and m in cl, "classes of 2, 3 and the class whose members are partners of each other"
        assert (s,) in cl and (d1,) in cl and (d2,) in cl and (x,) in cl, "S, D1, D2 and X are alone with their lists"
        assert not [g for g in cl if d1 in g and d2 in g] and not [g for g in cl if x in g and len(g) > 1]
        l1, l2, lx, lc = lists[d1], lists[d2], lists[x], lists[c2[0]]
        assert l1[0] == l2[0] and len(l1) == len(l2) and l1[:-1] == l2[:-1] and l1[-1] != l2[-1], "same first unit and length, last unit differs"
        assert lx[:len(lc)] == lc and len(lx) == len(lc) + 1, "equal but for one extra posting"
        assert sum(len(g) > 1 for g in cl) >= 3
        if (min_d, min_cov) == (1, 4) and max_d >= 3:
            got = _edge_set(nv)
            # every member of a class has the class's rows with its own first column ...
            for g in (c2, c3):
                assert len({frozenset(r_ for r_ in _rows_of(nv, a) if r_[1] not in g) for a in g}) == 1 and (1, p, 4) in _rows_of(nv, g[0])
            assert (3, c3[0], c3[1], 4) in got and (3, c3[1], c3[0], 4) in got
            # ... except where the partner is the member itself: M0 -> M1 and M1 -> M0 are edges, M0 -> M0 is not
            assert (2, m[0], m[1], 4) in got and (2, m[1], m[0], 4) in got
            assert not [e for e in got if e[1] == e[2]]
            assert _rows_of(nv, m[0]) - {(2, m[1], 4)} == _rows_of(nv, m[1]) - {(2, m[0], 4)}
            # S: its only slot that reaches min_cov is itself — no edge; a unique bit only if somebody selects it as b
            assert not _rows_of(nv, s) and s not in nv["unique"].tolist(), "S has no edge and no unique bit"
            # D1 reaches P four times, D2 three times: merged by mistake, D2 would get D1's row
            assert (1, p, 4) in _rows_of(nv, d1) and not [r_ for r_ in _rows_of(nv, d2) if r_[1] == p]
    elif name == "big":
        big = rk(BIG)
        assert big in cl and len(big) == CLASS_CAP + 1, "one list, cap + 1 k-mers"
        assert rk(BIG_T) in cl
        if min_cov <= 4 and min_d <= 1 <= max_d:
            (p,) = rk([BIG_P])
            assert all((1, p, 4) in _rows_of(nv, a) for a in big)
            assert all(len(_rows_of(nv, a)) > CLASS_CAP for a in rk(BIG_T)), "more rows per member than a table of 256 slots holds"
    else:
        g = rk((0, 1, 2))
        assert g in cl
        if min_cov <= 4 and min_d <= 1 <= max_d:
            assert all(len(_rows_of(nv, a)) >= 40 for a in g), "40 rows and more per member"
    c["classes"] = cl
    _cases[key] = c
    return c


# ------------------------------------------------------------------ the device against it
def _dist(engine, c, nv, what, n_parts=1, edge_cap=None):
    """The distance stage over `n_parts` partitions of the first k-mers; everything compared with the naive result."""
    engine.reset_unique()
    R = len(c["reads"])
    n_all = nv["edges"].shape[0]
    cap = n_all + 8 if edge_cap is None else edge_cap
    rows, ne, em = [], 0, 0
    for part in range(n_parts):
        n = engine.dist_edges(0, R, c["min_d"], c["max_d"], c["min_cov"], c["thr"], part, n_parts, edge_cap=cap)
        st = engine.stats()
        ne += n
        em += st["n_emissions"]
        rows.append(np.asarray(engine.edges(min(n, cap))).reshape(-1, 4))
    assert em == nv["E"], f"{what}: pair emissions {em} != {nv['E']}"
    assert ne == n_all, f"{what}: number of edges {ne} != {n_all}"
    got = pathcheck.sorted_edges(np.concatenate(rows)) if rows else np.zeros((0, 4), np.int64)
    if edge_cap is None:
        assert np.array_equal(got, nv["edges"]), f"{what}: A5 + A6 edges"
    else:      # the rows that fit are rows of the result, each once
        want = _edge_set(nv)
        mine = [tuple(int(v) for v in e) for e in got]
        assert n_parts > 1 or len(mine) == min(cap, n_all), what
        assert len(set(mine)) == len(mine) and set(mine) <= want, f"{what}: stored rows under a small edge_cap"
    assert np.array_equal(np.flatnonzero(engine.unique_mask()), nv["unique"]), f"{what}: unique k-mers"


def run(engine, c, knobs=None, n_parts=1, edge_cap=None, classes=(1, 0)):
    """A1 .. A3 once, then the distance stage under `knobs` with dist_classes 1 and 0.  Returns the stats of the run with the knob at 1."""
    nv, what = c["naive"], c["name"]
    engine.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    engine.count_kmers(c["k"])
    assert engine.select_rare(c["max_nonuniq"], c["lo"], c["hi"]) == len(nv["rare_kmers"])
    assert np.array_equal(engine.kmers(), nv["set_codes"])
    shapecheck._check_clouds(engine, nv, what)
    knobs = dict(knobs or {})
    stats = None
    for on in classes:
        with engine.knobs(**knobs, dist_classes=on):
            _dist(engine, c, nv, f"{what} {knobs} n_parts={n_parts} dist_classes={on}", n_parts, edge_cap)
            if on:
                stats = engine.stats()
    return stats


# small chunks of the edge output, a stage and a hot list that overflow: the rows of a member cross chunks, the late rows take the
# marked-slot sweep, the filter runs inside the bucket scan
TIGHT = dict(dist_edge_chunk=16, dist_stage=4, dist_hot_cap=8)
LAYOUTS = {k: stc.LAYOUTS[k] for k in ("wide", "regions26", "region_bytes", "one_workgroup")}


def repeated_rank_clouds(doubled=True):
    """Clouds for cf_set_clouds: five reads of 8 units, 120 ranks.  The ranks 0 and 2 stand in unit 0 of the reads 0 .. 2 and nowhere else —
    one posting list, a class of 2 — and rank 1 in unit 2 of the reads 0 and 1: TWICE in each of the two rows (doubled: the rows are not
    sets, cnt(0, 1, 2) = cnt(2, 1, 2) = 4, and the launch must form no class) or once (the same clouds as sets: cnt 2, no edge)."""
    rng = np.random.default_rng(14)
    n_kmers, per = 120, 8
    ent, cp = [], [0]
    for r in range(5):
        for u in range(per):
            row = np.sort(rng.choice(np.arange(3, n_kmers), 40, replace=False)).tolist()
            if u == 0 and r < 3:
                row = [0, 2] + row
            if u == 2 and r < 2:
                row = ([1, 1] if doubled else [1]) + row
            ent += row
            cp.append(len(ent))
    return np.arange(6, dtype=np.int64) * per, np.array(cp, np.int64), np.array(ent, np.int32), n_kmers


def prove_repeated_rank_clouds():
    """From numpy alone: as sets the clouds hold the class (0, 2) — fewer classes than first k-mers — and the doubled variant differs from them
    only by rows that are not strictly ascending.  Returns (fewest classes, first k-mers) of the set-like variant."""
    _, cp, ent, _ = repeated_rank_clouds(False)
    nv = dict(cloud_ptr=cp, entries=ent)
    assert (0, 2) in classes_of(nv), "the ranks 0 and 2 share one posting list"
    least, members = capped_classes(nv)
    assert least < members
    _, cp2, ent2, _ = repeated_rank_clouds(True)
    strictly = lambda c, e: all(np.all(np.diff(e[c[i]:c[i + 1]]) > 0) for i in range(c.size - 1))
    assert strictly(cp, ent) and not strictly(cp2, ent2)
    keep = np.ones(ent2.size, bool)
    keep[1:] = ~((ent2[1:] == ent2[:-1]) & (ent2[1:] == 1))
    assert np.array_equal(ent2[keep], ent), "the same clouds but for the second copy of rank 1"
    return least, members


def run_repeated_rank(engine, doubled=True):
    """The clouds above through cf_set_clouds with the knob at 1: the results are the oracle's, with the class (set-like rows) and without
    it (a rank twice in a row: the classes switch off on the device)."""
    prove_repeated_rank_clouds()
    with engine.knobs(dist_classes=1):
        edges = pathcheck.check_clouds(engine, *repeated_rank_clouds(doubled), 1, 150, 4, 0.8).tolist()
    assert ([2, 0, 1, 4] in edges and [2, 2, 1, 4] in edges) == doubled, "the edges that only the doubled rank makes"


def run_exchange(lib, rendezvous, knobs=None, n_reads=200):
    """Generator reads through the exchange path (the gathered view of the clouds) with the knob at its default, against the C oracle."""
    stc.run_exchange(lib, rendezvous, knobs, n_reads=n_reads)

"""The distance stage's set-up with groups: cf_group_walk_kernel — one wave cuts the runs of equal first units into groups
over windows of 64 positions whose lists it parks in LDS rows, and sums the members' own emissions on the way — and cf_group_fill_kernel
(a team of 32 lanes per group), on hand-built reads at the shapes where they can go wrong, against the plain restatement
shapecheck.naive_stage2 (edges, n_edges, n_emissions, unique mask: classcheck._dist) and the restated rule groupcheck.groups_of
(n_dist_passes: groupcheck.expected_passes).

Every case is built k-mer by k-mer (sketchtailcheck.reads_of).  The planted first k-mers of a case stand in ONE unit, the head unit H, so
they are one run of the sorted order keys; `before` reads of one unit in front of it, each with one k-mer of its own, are `before` runs
of one ahead of it: the run starts at position `before` of the order list, whatever the chunk borders are.  A planted k-mer's list is H
and the units it was put into beyond (unit 0 of two-unit reads: the pool); unit 1 of every such read holds the partner P, so
cnt(a, P, 1) is the LENGTH of a's list — a mask or a list that is wrong in one bit is a wrong count, a wrong edge or a wrong n_emissions.
Every case proves its shape FROM NUMPY ALONE before the device runs.
Used by test_emu_dist_setup.py (host emulator) and test_gpu_dist_setup.py (MI355X)."""
import numpy as np

import classcheck as cc
import groupcheck as gc
import shapecheck
import sketchtailcheck as stc

CHUNK = 64           # positions of the order list a wave of cf_group_walk_kernel owns
GROUP_MAX = gc.GROUP_MAX
CLASS_CAP = gc.CLASS_CAP
_cases = {}


class Builder:
    """Reads as lists of units as lists of k-mer numbers; numbers are handed out in ascending order, and every number is used, so
    (all k-mers being rare) a k-mer's rank is its number."""

    def __init__(self):
        self.layout, self.n_ids = [], 0

    def new(self, n=1):
        ids = list(range(self.n_ids, self.n_ids + n))
        self.n_ids += n
        return ids

    def read(self, n_units):
        self.layout.append([[] for _ in range(n_units)])
        return len(self.layout) - 1

    def put(self, x, r, u):
        self.layout[r][u].append(x)

    def finish(self, name, min_d, max_d, min_cov):
        for rd in self.layout:      # no unit is empty: a k-mer of its own where nothing was planted
            for unit in rd:
                if not unit:
                    unit += self.new()
        layout = [[sorted(u) for u in rd] for rd in self.layout]
        reads, units, texts = stc.reads_of(layout, self.n_ids, 53)
        R = len(reads)
        c = dict(name=f"setup: {name} min_d={min_d} max_d={max_d} min_cov={min_cov}", reads=reads, units=units, k=stc.K, max_nonuniq=10 * R, lo=1, hi=10 * R,
                 min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
        nv = shapecheck.naive_stage2(reads, units, stc.K, 10 * R, 1, 10 * R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
        nv["_unit_ptr"] = np.concatenate([[0], np.cumsum([len(u) for u in units])])
        assert len(nv["rare_kmers"]) == self.n_ids, "every k-mer is rare: ranks are numbers"
        c["naive"] = nv
        c["lists"] = cc.posting_lists(nv)
        c["unit_of"] = lambda r, u: int(nv["_unit_ptr"][r]) + u      # noqa: E731
        return c


def order_of(c, cap=GROUP_MAX, part=0, n_parts=1):
    """The order list of a partition as the restated rule has it: the members of its groups, one after the other."""
    return [x for g in gc.groups_of(c["naive"], cap, part, n_parts) for x in g[0]]


def runs_case(runs, before=0, pool=40, per=(1, 5), seed=7, min_d=1, max_d=150, min_cov=4, lists=None, name=None):
    """One run of planted first k-mers per entry of `runs` (its members), `before` runs of one in front of the first.  A member's list: its
    run's head unit and `per` = (lo, hi) units more, drawn from the run's pool of `pool` two-unit reads (unit 0); the partner P in unit 1
    of every read.  lists: {(run, member): pool indices} instead of the drawn ones."""
    key = ("runs", tuple(runs), before, pool, per, seed, min_d, max_d, min_cov, repr(lists))
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(seed)
    b = Builder()
    for _ in range(before):
        b.read(1)
    (P,) = b.new()
    planted, heads = [], []
    for i, n_mem in enumerate(runs):
        h = b.read(2)
        heads.append(h)
        b.put(P, h, 1)
        pool_reads = [b.read(2) for _ in range(pool)]
        for r in pool_reads:
            b.put(P, r, 1)
        mem = b.new(n_mem)
        planted.append(mem)
        for m, x in enumerate(mem):
            b.put(x, h, 0)
            if lists is not None and (i, m) in lists:
                chosen = lists[(i, m)]
            else:
                chosen = rng.choice(pool, int(rng.integers(per[0], per[1] + 1)), replace=False).tolist() if pool else []
            for q in sorted(chosen):
                b.put(x, pool_reads[q], 0)
    c = b.finish(name or f"runs {tuple(runs)} from position {before}", min_d, max_d, min_cov)
    c["planted"], c["P"] = planted, P
    order = order_of(c)
    for mem, h in zip(planted, heads):
        hu = c["unit_of"](h, 0)
        assert all(c["lists"][x][0] == hu for x in mem), "the members of a run share their first unit"
        first = min(order.index(x) for x in mem)
        assert sorted(order[first:first + len(mem)]) == sorted(mem), "... and stand next to each other"
    first0 = min(order.index(x) for x in planted[0])
    assert first0 == before, (first0, before)      # (P stands in unit 1 of the first head read: behind the first run)
    c["first_pos"] = [min(order.index(x) for x in mem) for mem in planted]
    _cases[key] = c
    return c


def border_case(n_mem, start):
    """A run of n_mem members with differing lists that starts at position `start` of the order list."""
    c = runs_case((n_mem,), before=start)
    lists = c["lists"]
    if n_mem > 1:
        assert len({lists[x] for x in c["planted"][0]}) > 1, "the lists differ"
    assert c["first_pos"][0] == start
    last = start + n_mem - 1
    c["chunks"] = (start // CHUNK, last // CHUNK)
    return c


def two_runs_case():
    """A run of one and a run of 40 that start in one chunk (between them the runs of one of the first run's pool)."""
    c = runs_case((1, 40), before=0, pool=12, name="runs of 1 and 40 in one chunk")
    p = c["first_pos"]
    assert p[0] // CHUNK == p[1] // CHUNK and (p[1] + 39) // CHUNK == p[1] // CHUNK, "two runs of very different length start and end in one chunk"
    return c


def chunk_end_case():
    """A run of 20 whose last member stands at position 63 of a chunk; position 0 of the next chunk is a run of one (the partner P)."""
    c = runs_case((20, 1), before=CHUNK - 20, pool=6, name="a run that ends at a chunk's last position, then a run of one")
    p, order, lists = c["first_pos"][0], order_of(c), c["lists"]
    assert (p + 20) % CHUNK == 0, "the run's last member is the chunk's last position"
    nxt, after = order[p + 20], order[p + 21]
    assert lists[nxt][0] != lists[order[p]][0] and lists[after][0] != lists[nxt][0], "the next chunk begins with a run of one"
    return c


def long_members_case():
    """300 members whose lists come from a pool of 20 units: no union passes 21 postings, so the union never closes a group and the cut at
    DIST_CLASS_CAP members falls inside what would be one group.  (With dist_group_cap 5 the same run is cut by the union again and again.)"""
    c = runs_case((300,), before=0, pool=20, per=(1, 4), name="a run of 300 members, unions below the cap")
    g = gc.groups_of(c["naive"])
    big = [x for x in g if set(x[0]) & set(c["planted"][0])]
    assert [len(x[0]) for x in big] == [CLASS_CAP, 300 - CLASS_CAP] and all(len(x[1]) <= 21 for x in big), "cut by the member cap alone"
    g5 = [x for x in gc.groups_of(c["naive"], 5) if set(x[0]) & set(c["planted"][0])]
    assert len(g5) > 20 and all(len(x[1]) <= 5 for x in g5)
    return c


def caps_case():
    """Lists at the caps, in ONE run (the second unit is the same for all, so the members stand in the order of their numbers):
      A    4 postings;  B33  33 postings — a group of its own that counts, BETWEEN A and C;  C  A's list and one more: A and C would share a
      group;  L32  32 postings: fits the lanes, a group of its own by the union;  L70  70 postings: the emission sum of a list longer than
      a wave;  then D16 (16) and D17 (the first of D16's and 16 more: the union reaches exactly 32 with it) and D1 (one posting more: 33, a new group)."""
    key = "caps"
    if key in _cases:
        return _cases[key]
    sets = [("A", [0, 1, 2]), ("B33", list(range(32))), ("C", [0, 1, 2, 3]), ("L32", [0] + list(range(40, 70))), ("L70", list(range(69))),
            ("D16", [0] + list(range(70, 84))), ("D17", [0] + list(range(84, 100))), ("D1", [0, 100])]
    c = runs_case((len(sets),), before=0, pool=101, lists={(0, m): s for m, (_, s) in enumerate(sets)}, name="lists and unions at the caps")
    ids = dict(zip([n for n, _ in sets], c["planted"][0]))
    lists, groups = c["lists"], gc.groups_of(c["naive"])
    L = {n: len(lists[x]) for n, x in ids.items()}
    assert (L["A"], L["B33"], L["C"], L["L32"], L["L70"], L["D16"], L["D17"], L["D1"]) == (4, 33, 5, 32, 70, 16, 18, 3), L
    gw = lambda n: gc.group_with(groups, ids[n])      # noqa: E731
    assert gw("A")[0] == (ids["A"],) and gw("B33") == ((ids["B33"],), (), True) and gw("C")[0][0] == ids["C"], "the counting group stands between A and C"
    assert len(set(lists[ids["A"]]) | set(lists[ids["C"]])) <= GROUP_MAX, "... which would otherwise share a group"
    assert gw("L32")[0] == (ids["L32"],) and len(gw("L32")[1]) == 32 and not gw("L32")[2], "a list of 32: a group by the union, not a counting one"
    assert gw("L70")[2], "70 postings: a counting group"
    assert gw("D16")[0] == (ids["D16"], ids["D17"]) and len(gw("D16")[1]) == 32, "a union that reaches exactly 32 with its last member"
    assert gw("D1")[0][0] == ids["D1"], "... and 33 with one more: the group closes"
    c["ids"] = ids
    _cases[key] = c
    return c


def emissions_case(min_d=2, max_d=5, min_cov=2):
    """Self pairs.  Five reads of 8 units; the planted k-mers stand in unit 0 of every read (one run: unit 0 of read 0) and again
      X[d]  in unit d of the same read, for d = min_d - 1 (where that is not unit 0 itself), min_d, max_d, max_d + 1: a self pair in every read exactly for min_d <= d <= max_d;
      T     in the units min_d and 2 min_d too: three times in one read (pairs at min_d, min_d and 2 min_d);
      B     in unit 7 — the last — of every read (unit 0 of the NEXT read is its neighbour in unit numbers — with min_d 1 a pair, if reads did not count; 7 > max_d: none inside).
    max_d is below the read's length."""
    key = ("emissions", min_d, max_d, min_cov)
    if key in _cases:
        return _cases[key]
    n_reads, n_units = 5, 8
    assert min_d >= 1 and max_d + 1 <= n_units - 1 and 2 * min_d <= max_d
    b = Builder()
    reads = [b.read(n_units) for _ in range(n_reads)]
    ds = [d for d in (min_d - 1, min_d, max_d, max_d + 1) if d >= 1]
    X = b.new(len(ds)); (T,) = b.new(); (B,) = b.new()
    for r in reads:
        for x, d in zip(X, ds):
            b.put(x, r, 0); b.put(x, r, d)
        for u in (0, min_d, 2 * min_d):
            b.put(T, r, u)
        b.put(B, r, 0); b.put(B, r, n_units - 1)
    c = b.finish("self pairs at the borders of [min_d, max_d]", min_d, max_d, min_cov)
    lists = c["lists"]
    assert len(lists[T]) == 3 * n_reads and all(len(lists[x]) == 2 * n_reads for x in X + [B])
    assert lists[B][1] + 1 == lists[B][2], "the last unit of a read and the first of the next: neighbouring unit numbers"
    assert len({lists[x][0] for x in X + [T, B]}) == 1, "one run"
    # the self pairs the library must subtract, restated: per k-mer the pairs of its postings in one read at a distance in [min_d, max_d]
    up = c["naive"]["_unit_ptr"]
    rd = lambda u: int(np.searchsorted(up, u, "right"))      # noqa: E731
    self_pairs = {x: sum(1 for i, u in enumerate(lists[x]) for v in lists[x][i + 1:] if rd(u) == rd(v) and min_d <= v - u <= max_d) for x in X + [T, B]}
    assert [self_pairs[x] for x in X] == [n_reads * (min_d <= d <= max_d) for d in ds] and sum(self_pairs[x] for x in X) == 2 * n_reads and self_pairs[T] == 3 * n_reads and self_pairs[B] == 0, self_pairs
    _cases[key] = c
    return c


def slice_border_case():
    """A self pair between the postings 7 and 8 of a list (cf_group_walk_kernel reads a list 8 postings to a team of lanes: the pair's two
    postings come from two loads).  Y stands in unit 0 of nine reads of four units and in unit 2 of the eighth; Z the same one read later (postings 8 and 9)."""
    key = "slice_border"
    if key in _cases:
        return _cases[key]
    b = Builder()
    reads = [b.read(4) for _ in range(10)]
    (Y,) = b.new(); (Z,) = b.new()
    for i, r in enumerate(reads[:9]):
        b.put(Y, r, 0)
    b.put(Y, reads[7], 2)
    for r in reads:
        b.put(Z, r, 0)
    b.put(Z, reads[8], 2)
    c = b.finish("a self pair across the border of two loads of one list", 1, 3, 4)
    lists = c["lists"]
    up = c["naive"]["_unit_ptr"]
    rd = lambda u: int(np.searchsorted(up, u, "right"))      # noqa: E731
    assert len(lists[Y]) == 10 and rd(lists[Y][7]) == rd(lists[Y][8]) and lists[Y][8] - lists[Y][7] == 2, "the postings 7 and 8 of Y are one read's"
    assert len(lists[Z]) == 11 and rd(lists[Z][8]) == rd(lists[Z][9]) and lists[Z][9] - lists[Z][8] == 2, "the postings 8 and 9 of Z too"
    _cases[key] = c
    return c


def long_run_case(n=2000):
    """One first unit shared by n first k-mers with small lists (one to three units more, out of 30)."""
    c = runs_case((n,), before=0, pool=30, per=(1, 3), seed=11, name=f"one first unit shared by {n} first k-mers")
    assert len(c["planted"][0]) == n and len({c["lists"][x][0] for x in c["planted"][0]}) == 1
    return c


# ------------------------------------------------------------------ the device against it
def check_passes(c, st, cap=GROUP_MAX, part=0, n_parts=1):
    """n_dist_passes of a launch whose tables did not split: the groups of the restated rule that have a partner unit."""
    if st["n_spilled"] == 0:
        want = gc.expected_passes(c, cap, part, n_parts)
        assert st["n_dist_passes"] == want, (c["name"], st["n_dist_passes"], want)


def run(engine, c, cap=GROUP_MAX, n_parts=1, groups=True):
    """A1 .. A3, then the distance stage with groups (dist_group_cap `cap`) over n_parts partitions: everything against the naive result, the
    passes of every partition against the restated rule."""
    nv, what = c["naive"], c["name"]
    engine.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    engine.count_kmers(c["k"])
    assert engine.select_rare(c["max_nonuniq"], c["lo"], c["hi"]) == len(nv["rare_kmers"])
    assert np.array_equal(engine.kmers(), nv["set_codes"])
    shapecheck._check_clouds(engine, nv, what)
    with engine.knobs(dist_groups=1, dist_group_cap=cap):
        cc._dist(engine, c, nv, f"{what} cap={cap} n_parts={n_parts}", n_parts)
        st = engine.stats()
    if groups:
        if n_parts == 1:
            check_passes(c, st, cap)
            if cap == GROUP_MAX and gc.mixed_groups(c, cap):
                gc.check_ran_in_groups(c, st, cap)
        else:      # (cc._dist leaves the stats of the last partition)
            check_passes(c, st, cap, n_parts - 1, n_parts)
    return st


BORDERS = [(n, s) for s in (0, 63) for n in (1, 63, 64, 65, 128, 129)]


def _border(n, s):
    def f(e):
        c = border_case(n, s)
        if (n, s) == (129, 63):
            assert c["chunks"] == (0, 2), "the run begins in one chunk and ends two chunks later"
        run(e, c)
    return f


def _min_cov_1(e):
    c = runs_case((65,), before=63, min_cov=1)
    run(e, c, groups=False)      # (no sketch, no groups: the classes' kernels, untouched, must still run)


CASES = {f"run_{n}_from_{s}": _border(n, s) for n, s in BORDERS}
CASES.update({
    "runs_1_and_40_in_one_chunk": lambda e: run(e, two_runs_case()),
    "run_ends_at_chunk_end": lambda e: run(e, chunk_end_case()),
    "run_300_member_cap": lambda e: run(e, long_members_case()),
    "run_300_group_cap_5": lambda e: run(e, long_members_case(), cap=5),
    "caps": lambda e: run(e, caps_case()),
    "caps_group_cap_5": lambda e: run(e, caps_case(), cap=5),
    "self_pairs_min_d_2": lambda e: run(e, emissions_case(2, 5)),
    "self_pairs_min_d_3": lambda e: run(e, emissions_case(3, 6, min_cov=4)),
    "self_pairs_min_d_1_across_reads": lambda e: run(e, emissions_case(1, 4)),
    "self_pair_across_two_loads": lambda e: run(e, slice_border_case()),
    "two_partitions": lambda e: run(e, border_case(129, 63), n_parts=2),
    "two_partitions_caps": lambda e: run(e, caps_case(), n_parts=2),
    "min_cov_1_classes_path": _min_cov_1,
    "long_run_2000": lambda e: run(e, long_run_case()),
})

"""The distance stage with the first k-mers of one first posting unit swept together, once, over the UNION of their posting lists (knob
dist_groups) on hand-built reads, against the plain restatement shapecheck.naive_stage2.

cnt(a, b, d) = #{u in L(a) : b in cloud(u + d)}.  The library cuts every run of first k-mers with one first unit into groups whose lists have
a union of at most dist_group_cap (<= 32) postings, sweeps the union into a table of 32-bit masks (which postings of the union brought the
pair), and member a_j with the list mask M_j reads cnt = popcount(mask & M_j) and its totals out of it.  The reads here are made of k-mers
chosen one by one (sketchtailcheck.reads_of), so a k-mer's posting list is exactly the units it was put into; unit 0 of read 0 — the
first unit of every planted list — holds planted k-mers only, so the runs and groups of a case are the ones it was built for.
Every case first proves FROM NUMPY ALONE (posting lists off the naive clouds, cut by groups_of below: the library's rule restated)
which groups it holds and what the naive result must show for them; then the device runs with the knob at 1 and at 0 and n_emissions,
n_edges, the edges as a sorted list and the unique mask are compared with the naive result.
Used by test_emu_dist_groups.py (host emulator) and test_gpu_dist_groups.py (MI355X)."""
import numpy as np

import classcheck as cc
import shapecheck
import sketchtailcheck as stc

GROUP_MAX = 32       # DIST_GROUP_MAX of cf_dist.hip: bits of a slot's mask
CLASS_CAP = cc.CLASS_CAP


# ------------------------------------------------------------------ the library's rule, restated
def groups_of(nv, cap=GROUP_MAX, part=0, n_parts=1, order_bits=16):
    """The groups of one partition's first k-mers: list of (ranks in order of joining, union as a list in order of joining, counting).
    Order inside a run of one first unit: the low `order_bits` bits of the second posting unit (the first one's for a list of one), then the rank."""
    lists = {x: us for x, us in cc.posting_lists(nv).items() if x % n_parts == part}
    key = lambda x: (lists[x][0], (lists[x][1] if len(lists[x]) > 1 else lists[x][0]) & ((1 << order_bits) - 1), x)      # noqa: E731
    out, cur, union, first = [], [], [], None
    for x in sorted(lists, key=key):
        L = lists[x]
        if len(L) > cap:
            if cur:
                out.append((tuple(cur), tuple(union), False))
            out.append(((x,), (), True))
            cur, union, first = [], [], None
            continue
        new = [u for u in L if u not in union]
        if not cur or L[0] != first or len(cur) == CLASS_CAP or len(union) + len(new) > cap:
            if cur:
                out.append((tuple(cur), tuple(union), False))
            cur, union, first, new = [], [], L[0], list(L)
        cur.append(x)
        union += new
    if cur:
        out.append((tuple(cur), tuple(union), False))
    return out


def group_with(groups, x):
    (g,) = [g for g in groups if x in g[0]]
    return g


def cnt_of(nv, a, b, d):
    """cnt(a, b, d) off the naive clouds."""
    cp, ent = nv["cloud_ptr"], nv["entries"]
    lists = cc.posting_lists(nv)
    n = 0
    for u in lists[a]:
        v = u + d
        if v < cp.size - 1 and _same_read(nv, u, v) and b in ent[cp[v]:cp[v + 1]].tolist():
            n += 1
    return n


def _same_read(nv, u, v):
    up = nv["_unit_ptr"]
    return np.searchsorted(up, u, "right") == np.searchsorted(up, v, "right")


def _with_unit_ptr(c):
    nv = c["naive"]
    if "_unit_ptr" not in nv:
        nv["_unit_ptr"] = np.concatenate([[0], np.cumsum([len(u) for u in c["units"]])])
    return nv


def expected_passes(c, cap=GROUP_MAX, part=0, n_parts=1):
    """Table passes of a launch WITH groups in which no table splits: one per group whose union (its own list, for a group that counts) has a
    partner unit.  Classes give more (one per distinct list): a launch that quietly fell back to them does not meet this number."""
    nv = _with_unit_ptr(c)
    lists = cc.posting_lists(nv)
    if c["max_d"] < max(c["min_d"], 1):
        return 0
    n = 0
    for members, union, counting in groups_of(nv, cap, part, n_parts):
        n += any(_same_read(nv, u, u + max(c["min_d"], 1)) for u in (lists[members[0]] if counting else union))
    return n


def mixed_groups(c, cap=GROUP_MAX):
    """The groups of a case that are more than a class: members with different lists (different masks over one union)."""
    nv = _with_unit_ptr(c)
    lists = cc.posting_lists(nv)
    return [g for g in groups_of(nv, cap) if len({lists[x] for x in g[0]}) > 1]


def check_ran_in_groups(c, st, cap=GROUP_MAX):
    """The launch swept groups, not classes: without a split table its passes are the groups the rule gives (at the full cap: fewer than the
    classes, with a group whose members differ)."""
    classes = len({us for us in cc.posting_lists(c["naive"]).values()})
    if cap == GROUP_MAX:
        assert mixed_groups(c, cap), "the case holds a group whose members differ"
        assert expected_passes(c, cap) < classes
    if st["n_spilled"] == 0:
        assert st["n_dist_passes"] == expected_passes(c, cap), (st["n_dist_passes"], expected_passes(c, cap), classes)


# ------------------------------------------------------------------ the read sets
N_READS, UNITS = 6, 7
# planted k-mers (numbers; their ranks follow their numbers) and the reads in whose unit 0 they stand — read 0 in every list
SUP, SUB, EQ2, W = 0, 1, 2, 3
IN_U0 = {SUP: (0, 1, 2, 3, 4), SUB: (0, 1, 2, 3), EQ2: (0, 1, 2, 3), W: (0, 3, 4, 5)}
E1, E2 = 4, 5            # share only the first unit: unit 0 of read 0, then unit 1 (E1) / unit 2 (E2) of the reads 1 .. 4
MM1, MM2 = 6, 7          # units 0 and 2 of the reads 0 .. 3: one list, each the other's selected partner at distance 2, and each twice in a read
PU, PO, PT = 8, 9, 10    # partners, see core_layout
N_PLANTED = 11


def core_layout(seed=41):
    """Six reads of seven units.
      PU  unit 1 of the reads 2, 3, 4, 5: cnt(., PU, 1) = 3 for SUP, 2 for SUB / EQ2, 3 for W — 4 in the union, min_cov in no member
      PO  unit 2 of the reads 0, 1, 2, 4: cnt(., PO, 2) = 4 for SUP alone (3 for SUB, 2 for W)
      PT  unit 3 of the reads 0 .. 3 and unit 5 of the reads 4, 5: for SUB cnt(3) = 4 and nothing else — selected; the union has 2 more at
          distance 5 (5 * 4 < 4 * 6): a total taken over the union would drop the edge.  SUP: 4 and 1 at distance 5 — 5 * 4 >= 4 * 5, selected."""
    rng = np.random.default_rng(seed)
    pool = np.arange(20, 140)
    layout = []
    for r in range(N_READS):
        rd = []
        for u in range(UNITS):
            unit = []
            if u == 0:
                unit += [x for x, rs in IN_U0.items() if r in rs]
                unit += [E1, E2] if r == 0 else []
                unit += [MM1, MM2] if r < 4 else []
            if u == 1:
                unit += ([E1] if 1 <= r <= 4 else []) + ([PU] if r >= 2 else [])
            if u == 2:
                unit += ([E2] if 1 <= r <= 4 else []) + ([MM1, MM2] if r < 4 else []) + ([PO] if r in (0, 1, 2, 4) else [])
            if u == 3 and r < 4:
                unit += [PT]
            if u == 5 and r >= 4:
                unit += [PT]
            rd.append(stc._fill(rng, unit, len(unit) + (0 if (r, u) == (0, 0) else 5), pool))
        layout.append(rd)
    return layout, 140


A16, A17, B33, P33 = 0, 1, 2, 3


def union_layout(extra):
    """33 + extra reads of two units.  A16: unit 0 of the reads 0 .. 15; A17: unit 0 of the reads 0, 1 and 16 .. 31 (+ read 32 with extra = 1; read 1 puts it behind A16 and in front of B33 in the run):
    the union has exactly 32 postings (one group at the cap) or 33 (the group closes).  B33: unit 0 of the reads 0 .. 32 — 33 postings, more
    than a mask has bits: a group of its own that counts.  P33 in unit 1 of every read."""
    rng = np.random.default_rng(42)
    pool = np.arange(10, 60)
    layout = []
    for r in range(33 + extra):
        u0 = ([A16] if r < 16 else []) + ([A17] if r <= 1 or 16 <= r < 32 + extra else []) + ([B33] if r < 33 else [])
        layout.append([stc._fill(rng, u0, len(u0) + (0 if r == 0 else 3), pool), stc._fill(rng, [P33], 4, pool)])
    return layout, 60


_cases = {}


def case(name, min_d=1, max_d=150, min_cov=4):
    key = (name, min_d, max_d, min_cov)
    if key in _cases:
        return _cases[key]
    layout, n_ids = {"core": core_layout, "u32": lambda: union_layout(0), "u33": lambda: union_layout(1)}[name]()
    reads, units, texts = stc.reads_of(layout, n_ids, 43)
    R = len(reads)
    c = dict(name=f"groups:{name} min_d={min_d} max_d={max_d} min_cov={min_cov}", reads=reads, units=units, k=stc.K, max_nonuniq=R, lo=1, hi=R,
             min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv = shapecheck.naive_stage2(reads, units, stc.K, R, 1, R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv["_unit_ptr"] = np.concatenate([[0], np.cumsum([len(u) for u in units])])
    c["naive"] = nv
    rk = lambda ids: tuple(stc._ranks(nv, texts, list(ids)))      # noqa: E731
    lists = cc.posting_lists(nv)
    groups = groups_of(nv)
    c["groups"] = groups
    rows = lambda a: cc._rows_of(nv, a)      # noqa: E731
    if name == "core":
        sup, sub, eq2, w, e1, e2, m1, m2, pu, po, pt = rk(range(N_PLANTED))
        planted = (sup, sub, eq2, w, e1, e2, m1, m2)
        g = group_with(groups, sup)
        assert set(planted) <= set(g[0]) and not g[2], "the planted first k-mers form ONE group at the cap of 32"
        assert len(g[1]) == 6 + 4 + 5 and len({lists[x][0] for x in planted}) == 1, "union: unit 0 of six reads, unit 1 of four, unit 2 of five"
        assert set(lists[sub]) < set(lists[sup]), "a member that is a strict subset of another"
        assert set(lists[e1]) & set(lists[e2]) == {lists[e1][0]}, "two members that share only the first unit"
        assert lists[sub] == lists[eq2] and lists[m1] == lists[m2], "members with equal lists"
        for cap in (2, 5):
            gs = groups_of(nv, cap)
            assert all(len(x[1]) <= cap for x in gs) and len(gs) > len(groups), "a smaller cap closes groups earlier"
            assert group_with(gs, m1)[2] and group_with(gs, m1)[0] == (m1,), "8 postings above the cap: a counting group of one"
        if (min_d, min_cov) == (1, 4) and max_d >= 5:
            union_cnt = len([u for u in g[1] if _same_read(nv, u, u + 1) and pu in nv["entries"][nv["cloud_ptr"][u + 1]:nv["cloud_ptr"][u + 2]].tolist()])
            assert union_cnt >= 4 and max(cnt_of(nv, a, pu, 1) for a in planted) == 3, "PU reaches min_cov in the union and in no member"
            assert not [a for a in planted if [r_ for r_ in rows(a) if r_[1] == pu]] and pu not in nv["unique"].tolist(), "... no edge and no unique bit"
            assert [a for a in planted if (2, po, 4) in rows(a)] == [sup], "PO reaches min_cov in exactly one member"
            assert (3, pt, 4) in rows(sub) and (3, pt, 4) in rows(eq2) and (3, pt, 4) in rows(sup), "PT: selected with the member's own total"
            tot_union = sum(1 for u in g[1] for d in (3, 5) if u + d < nv["cloud_ptr"].size - 1 and _same_read(nv, u, u + d)
                            and pt in nv["entries"][nv["cloud_ptr"][u + d]:nv["cloud_ptr"][u + d + 1]].tolist())
            assert 5 * 4 < 4 * tot_union, "... which the union's total would drop"
            assert (2, m2, 4) in rows(m1) and (2, m1, 4) in rows(m2) and not [e for e in cc._edge_set(nv) if e[1] == e[2]], "partners of each other, never of themselves"
    else:
        a16, a17, b33, p33 = rk((A16, A17, B33, P33))
        assert len(lists[a16]) == 16 and len(lists[b33]) == 33 and lists[a16][0] == lists[a17][0] == lists[b33][0]
        ga, gb = group_with(groups, a16), group_with(groups, b33)
        assert gb == ((b33,), (), True), "33 postings: a group of its own that counts"
        if name == "u32":
            assert len(lists[a17]) == 18 and set(ga[0]) == {a16, a17} and len(ga[1]) == 32, "a union of exactly 32 postings: one group"
        else:
            assert len(lists[a17]) == 19 and ga[0] == (a16,) and group_with(groups, a17)[0] == (a17,), "a union of 33: the group closes"
        if min_cov <= 4 and min_d <= 1 <= max_d:
            assert (1, p33, 16) in rows(a16) and (1, p33, len(lists[a17])) in rows(a17) and (1, p33, 33) in rows(b33)
    _cases[key] = c
    return c


# ------------------------------------------------------------------ the device against it
def run(engine, c, knobs=None, n_parts=1, edge_cap=None, groups=(1, 0)):
    """A1 .. A3 once, then the distance stage under `knobs` with dist_groups 1 and 0.  Returns the stats of the run with the knob at 1.
    (c: a case of this module, of classcheck or of sketchtailcheck — they share their form.)"""
    nv, what = c["naive"], c["name"]
    engine.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    engine.count_kmers(c["k"])
    assert engine.select_rare(c["max_nonuniq"], c["lo"], c["hi"]) == len(nv["rare_kmers"])
    assert np.array_equal(engine.kmers(), nv["set_codes"])
    shapecheck._check_clouds(engine, nv, what)
    knobs = dict(knobs or {})
    stats = None
    for on in groups:
        with engine.knobs(**knobs, dist_groups=on):
            cc._dist(engine, c, nv, f"{what} {knobs} n_parts={n_parts} dist_groups={on}", n_parts, edge_cap)
            if on:
                stats = engine.stats()
    return stats


TIGHT = cc.TIGHT
LAYOUTS = cc.LAYOUTS


def run_repeated_rank(engine, doubled=True):
    """classcheck.repeated_rank_clouds through cf_set_clouds with the knob at 1: a rank twice in a row makes every first k-mer a group that counts."""
    with engine.knobs(dist_groups=1):
        cc.run_repeated_rank(engine, doubled)


def run_exchange(lib, rendezvous, knobs=None, n_reads=250):
    """Generator reads through the exchange path (the gathered view of the clouds) with the knob at its default, against the C oracle."""
    stc.run_exchange(lib, rendezvous, knobs, n_reads=n_reads)

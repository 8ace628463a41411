"""The distance kernel's filter over ALL members of a group in one section (knob dist_filter_once) on hand-built reads,
against the plain restatement shapecheck.naive_stage2.

With the knob at 1 a thread of the mask table's filter keeps its hot slot and the masks of its b in registers, loops over the members
of the group (32 to a batch) and the rows are reserved once per batch; with 0 the launch filters member by member, as it did before.
Both must give the naive result: n_emissions, n_edges, the edges as a sorted list, the unique mask (classcheck._dist compares them).
The reads are made k-mer by k-mer (sketchtailcheck.reads_of), and every case proves its regime FROM NUMPY ALONE before the device runs.
Used by test_emu_dist_member_filter.py (host emulator) and test_gpu_dist_member_filter.py (MI355X)."""
import numpy as np

import classcheck as cc
import groupcheck as gc
import shapecheck
import sketchtailcheck as stc

BATCH = 32      # members to a batch of the section: a bit each in a lane's selection word

_cases = {}


def flat(n_first, n_partners, n_reads=5, min_cov=4):
    """n_reads reads of two units: the first k-mers 0 .. n_first - 1 in unit 0 of every read (equal lists: ONE group of n_first members),
    the partners in unit 1 of every read.  cnt(a, p, 1) = n_reads for every pair and nothing else: n_first * n_partners rows, and the
    group's hot list has n_partners slots."""
    key = ("flat", n_first, n_partners, n_reads, min_cov)
    if key in _cases:
        return _cases[key]
    first, partners = list(range(n_first)), list(range(n_first, n_first + n_partners))
    layout = [[first, partners] for _ in range(n_reads)]
    c = _case(f"member filter: flat {n_first} x {n_partners}", layout, n_first + n_partners, min_cov)
    nv, rk = c["naive"], c["rk"]
    fr, pr = rk(first), rk(partners)
    assert n_reads >= min_cov
    g = gc.group_with(c["groups"], fr[0])
    assert set(g[0]) == set(fr) and not g[2], "the first k-mers form one group that does not count"
    assert nv["edges"].shape[0] == n_first * n_partners
    assert all((1, p, n_reads) in cc._rows_of(nv, a) for a in (fr[0], fr[-1]) for p in (pr[0], pr[-1]))
    return c


def quiet(min_cov=4, n_reads=5):
    """Two runs of first k-mers: L (unit 0 of every read, partners in unit 1 of every read: rows) and Q (unit 2 of every read; unit 3 holds
    k-mers that occur in ONE read each).  Q has min_cov postings with a partner unit, so its sweeps run, and no pair of Q reaches min_cov:
    a group without a single hot slot between groups that have rows.  (The section must still meet the workgroup once: the next first
    k-mer's head is published in front of it.)"""
    key = ("quiet", min_cov, n_reads)
    if key in _cases:
        return _cases[key]
    L, P, Q = [0, 1, 2], [3, 4, 5, 6], [7, 8, 9]
    nid = 10
    layout = []
    for r in range(n_reads):
        once = list(range(nid, nid + 6)); nid += 6
        layout.append([L, P, Q, once])
    c = _case("member filter: quiet group", layout, nid, min_cov)
    nv, rk = c["naive"], c["rk"]
    for q in rk(Q):
        assert len(cc.posting_lists(nv)[q]) == n_reads >= min_cov and not cc._rows_of(nv, q), "swept, nothing selected"
    assert all(len(cc._rows_of(nv, a)) >= len(P) for a in rk(L))
    return c


MEMBER_KEYS = 8      # DIST_MEMBER_KEYS of cf_dist.hip: masks of one b that a thread keeps in registers


def _home(b, n_buckets):
    """The home bucket of b in the 4-key-bucket tables of cf_dist.hip (cf_tab_narrow_t::hash, ::home), restated."""
    h = ((b & 0xFFFFFF) * 0x9E3779) & 0xFFFFFFFF
    return ((h >> 16) * (n_buckets & 0xFFFF)) >> 16


WRAP_SLOTS = 256      # the smallest table: 64 buckets of four keys


def keys(n_keys, min_cov=4, wrap=False):
    """One b at exactly n_keys distances from a group of two first k-mers with equal lists (A1, A2: unit 0 of every read): at distance 1 in
    every read (cnt = c), at the distances 2 .. n_keys in one read each.  c is chosen so that 5 c >= 4 total FAILS with every key summed
    (total = c + n_keys - 1) and HOLDS with one single missed: the edge (A, b, 1) must not be there, and a total over too few keys makes it.
    n_keys = MEMBER_KEYS: the registers hold them all; MEMBER_KEYS + 1: the slot walks the chain per member.  More than four keys of one b
    never fit its home bucket, so the totals come from the chain walk.
    wrap: b is given the number whose rank has the LAST bucket of a table of WRAP_SLOTS slots as its home: the chain of its keys goes on in
    bucket 0 (run with dist_slots = WRAP_SLOTS)."""
    key = ("keys", n_keys, min_cov, wrap)
    if key in _cases:
        return _cases[key]
    singles = n_keys - 1
    c = 4 * singles - 2      # 5 c < 4 (c + singles)  <=>  c < 4 singles;   5 c >= 4 (c + singles - 1)  <=>  c >= 4 singles - 4
    assert 5 * c < 4 * (c + singles) and 5 * c >= 4 * (c + singles - 1) and c <= gc.GROUP_MAX, "the union of the group fits a mask"
    A1, A2, B = 0, 1, 2
    n_ids = 3 + 2 * c * n_keys
    if wrap:      # (every number is used and every k-mer is rare, so a k-mer's rank is its number)
        B = next(x for x in range(2, n_ids) if _home(x, WRAP_SLOTS // 4) == WRAP_SLOTS // 4 - 1)
    free = iter(x for x in range(2, n_ids) if x != B)
    layout = []
    for r in range(c):
        rd = []
        for u in range(n_keys + 1):
            unit = [A1, A2] if u == 0 else ([B] if u == 1 or (u >= 2 and r == u - 2) else [])
            if u:      # (two k-mers of its own in every unit behind the first: no unit is empty, nothing else repeats, and unit 0 holds the group alone)
                unit = unit + [next(free), next(free)]
            rd.append(sorted(unit))
        layout.append(rd)
    cs = _case(f"member filter: one b at {n_keys} distances{' (wrapping chain)' if wrap else ''}", layout, n_ids, min_cov)
    nv, rk = cs["naive"], cs["rk"]
    a1, a2, b = rk((A1, A2, B))
    g = gc.group_with(cs["groups"], a1)
    assert set(g[0]) == {a1, a2} and not g[2]
    cnts = [gc.cnt_of(nv, a1, b, d) for d in range(1, n_keys + 2)]
    assert cnts == [c] + [1] * singles + [0], cnts
    assert not [r_ for a in (a1, a2) for r_ in cc._rows_of(nv, a) if r_[1] == b], "dominance fails with the whole total: no edge to b"
    if wrap:
        assert _home(b, WRAP_SLOTS // 4) == WRAP_SLOTS // 4 - 1 and n_keys > 4, "b's keys begin in the last bucket and do not fit it"
    _cases[key] = cs
    return cs


def self_only(min_cov=4):
    """A group of two with different lists, X and Y (both in unit 0 of read 0).  X: unit 0 AND unit 1 of the reads 0 .. 4 — cnt(X, X, 1) = 5, the
    only pair of X that reaches min_cov is X itself: no row, and no unique bit (X is nobody's partner either: cnt(Y, X, 1) = 1).  Y: unit 0 of
    the reads 0 and 5 .. 8, with P in unit 1 of the reads 5 .. 8: the row (Y, P, 1, 4)."""
    key = ("self_only", min_cov)
    if key in _cases:
        return _cases[key]
    X, Y, P = 0, 1, 2
    nid = 3
    layout = []
    for r in range(9):
        u0 = [X, Y] if r == 0 else ([X] if r <= 4 else [Y])
        u1 = ([X] if r <= 4 else [P]) + [nid, nid + 1]; nid += 2
        layout.append([u0, sorted(u1)])
    cs = _case("member filter: a member whose only hot slot is itself", layout, nid, min_cov)
    nv, rk = cs["naive"], cs["rk"]
    x, y, p_ = rk((X, Y, P))
    g = gc.group_with(cs["groups"], x)
    assert set(g[0]) == {x, y} and not g[2], "one group, no counting"
    assert gc.cnt_of(nv, x, x, 1) == 5 >= min_cov and gc.cnt_of(nv, y, x, 1) == 1 and gc.cnt_of(nv, y, p_, 1) == 4 >= min_cov
    assert not cc._rows_of(nv, x) and (1, p_, 4) in cc._rows_of(nv, y)
    uq = set(np.asarray(nv["unique"]).tolist())
    assert x not in uq and y in uq and p_ in uq, "no unique bit for the member without a row"
    _cases[key] = cs
    return cs


N_BLOCKS, BLOCK_KMERS = 8, 20


def many_chunks(min_cov=4):
    """Five equal reads of eight units of 20 k-mers of their own: the first k-mers of unit g are one group of 20 whose rows are every k-mer of
    the units behind it (20 * 20 * (7 - g) rows), eight heads for the kernel's eight ticket queues.  With chunks of 16 rows, in the launch
    shape the library picks, each group reserves dozens of chunks while the others do the same: a group's reservations are NOT one behind the other, and a
    row beyond the chunk's remainder that is written past the old chunk lands in another workgroup's rows.  (On a device only: the host
    emulator runs the workgroups one after the other, and there the chunks of a launch are contiguous.)"""
    key = ("many_chunks", min_cov)
    if key in _cases:
        return _cases[key]
    layout = [[list(range(BLOCK_KMERS * g, BLOCK_KMERS * (g + 1))) for g in range(N_BLOCKS)] for _ in range(5)]
    cs = _case("member filter: many chunks, many workgroups", layout, N_BLOCKS * BLOCK_KMERS, min_cov)
    nv, rk = cs["naive"], cs["rk"]
    big = 0
    for g in range(N_BLOCKS - 1):
        fr = rk(range(BLOCK_KMERS * g, BLOCK_KMERS * (g + 1)))
        assert set(gc.group_with(cs["groups"], fr[0])[0]) == set(fr)
        rows = sum(len(cc._rows_of(nv, a)) for a in fr)
        assert rows == BLOCK_KMERS * BLOCK_KMERS * (N_BLOCKS - 1 - g)
        big += rows >= 40 * 16
    assert big >= 6, "six groups and more with 40 chunks of 16 rows and more each"
    _cases[key] = cs
    return cs


def _case(name, layout, n_ids, min_cov, min_d=1, max_d=150):
    reads, units, texts = stc.reads_of(layout, n_ids, 47)
    R = len(reads)
    c = dict(name=f"{name} min_cov={min_cov}", reads=reads, units=units, k=stc.K, max_nonuniq=10 * R, lo=1, hi=10 * R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv = shapecheck.naive_stage2(reads, units, stc.K, 10 * R, 1, 10 * R, min_d=min_d, max_d=max_d, min_cov=min_cov, thr=0.8)
    nv["_unit_ptr"] = np.concatenate([[0], np.cumsum([len(u) for u in units])])
    c["naive"] = nv
    c["rk"] = lambda ids: tuple(stc._ranks(nv, texts, list(ids)))      # noqa: E731
    c["groups"] = gc.groups_of(nv)
    _cases[(name, min_cov)] = c
    return c


def run(engine, c, knobs=None, n_parts=1, edge_cap=None, once=(1, 0)):
    """A1 .. A3 once, then the distance stage under `knobs` with dist_filter_once 1 and 0 (groups on).  Returns the stats per setting."""
    nv, what = c["naive"], c["name"]
    engine.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    engine.count_kmers(c["k"])
    assert engine.select_rare(c["max_nonuniq"], c["lo"], c["hi"]) == len(nv["rare_kmers"])
    assert np.array_equal(engine.kmers(), nv["set_codes"])
    shapecheck._check_clouds(engine, nv, what)
    knobs = dict(knobs or {})
    stats = {}
    for on in once:
        with engine.knobs(**knobs, dist_groups=1, dist_filter_once=on):
            cc._dist(engine, c, nv, f"{what} {knobs} n_parts={n_parts} dist_filter_once={on}", n_parts, edge_cap)
            stats[on] = engine.stats()
    return stats


def _core(min_cov):
    return lambda e: run(e, gc.case("core", min_cov=min_cov))


CASES = {
    # a pair that reaches min_cov in the union and in no member / in exactly one; a total that holds with the member's own sum only; partners of each other
    "core_min_cov_2": _core(2),
    "core_min_cov_4": _core(4),
    # 120 rows of one group over chunks of 16 rows: the rows of a batch cross several chunk borders and exceed a chunk; then rows beyond the cap
    "rows_chunk_16": lambda e: run(e, cc.case("rows"), dict(dist_edge_chunk=16)),
    "rows_edge_cap_50": lambda e: run(e, cc.case("rows"), dict(dist_edge_chunk=16), edge_cap=50),
    # the batch borders
    "members_32": lambda e: run(e, flat(32, 3)),
    "members_33": lambda e: run(e, flat(33, 3)),
    "members_64": lambda e: run(e, flat(64, 3)),
    "members_65": lambda e: run(e, flat(65, 3)),
    "members_256": lambda e: run(e, cc.case("big")),
    # a hot list longer than the workgroup (150 slots, 128 threads: a thread takes two); with a list cap of 8 the list overflows, the scan's
    # list overflows too (150 > 8) and the launch filters member by member whatever the knob says: the fall-back
    "hot_150_block_128": lambda e: run(e, flat(3, 150), dict(dist_block=128)),
    "hot_150_cap_8": lambda e: run(e, flat(3, 150), dict(dist_block=128, dist_hot_cap=8)),
    # ... and with no first k-mer keeping the inserts' list (dist_hot_entries 0): the filter's scan makes the list, over the insert queues, and
    # its 150 slots fit it — the section reads the scan's list
    "hot_150_scan": lambda e: run(e, flat(3, 150), dict(dist_block=128, dist_hot_entries=0)),
    # one b at as many distances as a thread keeps masks in registers, and at one more (the walk per member): the total must be the whole one
    "keys_K": lambda e: run(e, keys(MEMBER_KEYS)),
    "keys_K_plus_1": lambda e: run(e, keys(MEMBER_KEYS + 1)),
    # the same with b's chain beginning in the last bucket of the table: the walk goes on in bucket 0
    "keys_K_wrap": lambda e: run(e, keys(MEMBER_KEYS, wrap=True), dict(dist_slots=WRAP_SLOTS)),
    "keys_K_plus_1_wrap": lambda e: run(e, keys(MEMBER_KEYS + 1, wrap=True), dict(dist_slots=WRAP_SLOTS)),
    # a member whose only hot slot is itself: no row, no unique bit, while the other member has its row
    "self_only": lambda e: run(e, self_only()),
    # rows of several groups over chunks of 16 rows, reserved by several workgroups at the same time
    "many_chunks": lambda e: run(e, many_chunks(), dict(dist_edge_chunk=16)),
    # a union table that splits: rows of one group from more than one pass
    "split_table": lambda e: _split(e),
    # a group without a hot slot between groups with rows
    "quiet_group": lambda e: run(e, quiet()),
    # a counting head (33 postings: more than a mask has bits)
    "counting_u33": lambda e: run(e, gc.case("u33")),
    # min_cov 1: no sketch and no groups — the class instance runs, the knob must not matter
    "min_cov_1": _core(1),
    "two_partitions": lambda e: run(e, gc.case("core"), n_parts=2),
    "one_workgroup": lambda e: run(e, gc.case("core"), gc.LAYOUTS["one_workgroup"]),
}


def _split(e):
    c = flat(3, 200)
    st = run(e, c, dict(dist_slots=256))
    assert st[1]["n_spilled"] > 0 and st[0]["n_spilled"] > 0, "200 keys do not fit 70 % of 256 slots: the table splits"

"""The distance kernel's three LOSSY structures, with the collisions planted: the counting sketch (4-bit or 8-bit counters under a hash of
(b, d)), the bitmap of marked b (one bit per rank mod 65536) and the exact table that is split by hash bits of b when it fills.  Each
is right only because a collision adds work and never loses a pair; every case here makes a collision certain and SELECTS the pair
that the collision would lose.

No case restates a hash.  Family 1 makes a shared sketch counter certain by counting: V victims and B bursts under one first k-mer
with V * B / C >= 16 for the C counters of the launch (at most 262 144 of four bits, 131 072 bytes), so that for any hash that spreads the chance that no victim
shares a counter with a burst is below exp(-16).  Family 2 uses the one thing the bitmap documents about itself — ranks that are equal
mod 65536 share a bit.  Family 3 uses the one thing the split documents — it goes by bits of b, so the keys of ONE b stay together.
Every input is a fixed list of ranks (no RNG); every expectation is the oracle's (recruit.dist_histogram + filter_edges through
pathcheck.check_clouds and countcheck.run).  DESIGN.md 11 has the table of planted faults that each case turns red.
Used by test_emu_dist_collisions.py (host emulator) and test_gpu_dist_collisions.py (MI355X)."""
import re

import pytest

import countcheck as cc
import pathcheck
from centroflye_amd.engine import DeviceError

REFUSED_SPLIT = r"\(-34\).*could not be partitioned far enough"

_cases = {}


def _case(key, make):
    if key not in _cases:
        c = make()
        c["hist"] = pathcheck.clouds_histogram(*c["clouds"], c["min_d"], c["max_d"])
        _cases[key] = c
    return _cases[key]


def _run(engine, c, min_cov, knobs):
    """countcheck.run; None when the forced region layout refuses the input (the only refusal a layout knob may answer with)."""
    try:
        return cc.run(engine, c, min_cov, knobs)
    except DeviceError as e:
        if "dist_regions" in knobs and re.search(cc.REFUSED_REGIONS, str(e)):
            return None
        raise


# ------------------------------------------------------------------ family 1: a victim pair shares a sketch counter with a burst
V, ROW = 4096, 256      # victims, entries of a partner row
V_ROWS = V // ROW
COUNTERS = {16: 262144, 254: 131072, 255: 131072}      # by the burst that wraps them: the most 4-bit counters / bytes a launch can have


def n_bursts(n):
    return 16 * COUNTERS[n] // V      # 1024 bursts of 16, 512 of 254 or 255: V * B / C = 16


# The ranks: the powers of 75 mod 65537 (a primitive root: 65536 distinct values, none of them 0) in their order — a fixed list with no
# pattern that a multiplicative hash could lay out evenly, as it does with ranks in steps of 16 (tried first: not one collision).
RANKS = [75]
while len(RANKS) < V + n_bursts(16):
    RANKS.append(RANKS[-1] * 75 % 65537)
F1_MIN_D, F1_MAX_D = V_ROWS, 2 * V_ROWS - 1      # rows at the units 16 .. 31 of a read: row against row is at most 15 apart and not counted

# (min_cov, n, k): a burst of n equal entries, k of the victims' reads in front of the bursts
FOUR_BIT = ((8, 16, 4), (9, 16, 4), (9, 16, 5))      # the counter stands at k; 16 adds see k .. 15, 0 .. k - 1; those that saw 12 .. 15 go back: 0 (k = 4) or 1 (k = 5)
BYTES = ((10, 255, 5), (10, 254, 5), (12, 255, 5), (12, 254, 5))      # k + n wraps the byte to k - 1 or k - 2 (256 would put it back where it was)
BYTES_AT_9 = ((9, 255, 5), (9, 254, 5))      # the same under dist_sketch_bits=8
BOTH = ((9, 255, 4),)      # default bits: the 4-bit sweep wraps, the byte sweep wraps, every b is marked

F1_SETTINGS = {
    "one_wave": dict(dist_block=64),      # one wave sweeps the items of the first k-mer in order
    "one_wave_small_table": dict(dist_block=64, dist_slots=256),      # (far fewer counters; the table of the marked b splits)
    "default": {},      # the waves interleave on a device: any order must give the oracle's result
    "no_groups": dict(dist_groups=0),
    "no_classes": dict(dist_classes=0),
    "wide": dict(dist_wide=1),
    "regions": dict(dist_regions=2),
    "no_sketch": dict(dist_sketch=0),      # the control
}


def victim_case(min_cov, n, k, short=False):
    """The first k-mer 0 with V victim partners and B burst partners.
    A victims' read: 0 in unit 0, the victims in rows of ROW at the units 16 .. 31 (victim i at distance 16 + i // ROW; the first row
    at the bursts' own distance) — every read serves every victim, and cnt(0, x_i, d_i) is the number of such reads: min_cov exactly
    (short: min_cov - 1, and no victim may be selected — a false mark must not select).
    A burst's read: 0 in unit 0, the burst's rank n times in unit 16: n adds to one counter out of one wave step.
    Order: k victims' reads, the B bursts' reads, the other victims' reads — posting order, which is item order for these clouds (a
    row with repeats is not a set: no tail items, no reordering).
    Victims are the first V of RANKS (all over the bitmap), bursts the ones behind them."""
    def make():
        cnt = min_cov - bool(short)
        assert 0 < k < cnt and n >= min_cov
        victims, bursts = RANKS[:V], RANKS[V:V + n_bursts(n)]
        assert len(set(RANKS)) == len(RANKS) and 0 not in RANKS
        gap = [[] for _ in range(F1_MIN_D - 1)]
        v_read = [[0]] + gap + [victims[r * ROW:(r + 1) * ROW] for r in range(V_ROWS)]
        reads = [v_read] * k + [[[0]] + gap + [[r] * n] for r in bursts] + [v_read] * (cnt - k)
        pairs = [(0, x, F1_MIN_D + i // ROW, cnt) for i, x in enumerate(victims)] + [(0, r, F1_MIN_D, n) for r in bursts]
        return dict(name=f"{V} victims at {cnt} ({k} in front) and {len(bursts)} bursts of {n}", clouds=cc.build(reads), pairs=pairs, min_d=F1_MIN_D, max_d=F1_MAX_D)
    return _case(("victims", min_cov, n, k, short), make)


def run_victims(engine, min_cov, n, k, settings=F1_SETTINGS, extra=None, short=False):
    """Every victim is selected with the count min_cov and every burst pair with its n (countcheck.run: pair by pair, from the oracle's
    rows) — or, short, no victim is.  Which path ran, from the passes (cf_stats names no path): the case has ONE first k-mer with
    partners, so one pass — unless the table was split, or every b was marked and the passes were set up for all the partner entries."""
    c = victim_case(min_cov, n, k, short)
    assert sorted({p[3] for p in c["pairs"]}) == sorted({min_cov - bool(short), n})
    heads, stats = 1, {}
    for name, knobs in settings.items():
        knobs = dict(knobs, **(extra or {}))
        st = stats[name] = _run(engine, c, min_cov, knobs)
        if st is None:
            continue
        sketch = knobs.get("dist_sketch", 1)
        in_bytes = min_cov >= 10 or knobs.get("dist_sketch_bits") == 8
        if sketch and n >= 254 and knobs.get("dist_block") == 64 and st["n_spilled"] == 0:
            # a burst of 254 or 255 wraps no byte by itself: a victim's adds lay in its counter.  The wrap has sent the first k-mer to "every
            # b marked", which sets up partitions for ALL its partner entries: twenty tables' worth and more, the 256-unit table or not
            assert st["n_dist_passes"] > heads, f"{name}, {c['name']}: every b marked, in one partition? {st}"
        if sketch and n == 16 and not in_bytes and knobs.get("dist_block") == 64 and "dist_slots" not in knobs and st["n_spilled"] == 0:
            # 16 adds wrap four bits and no byte: the second sweep, with bytes, is clean, the marked b fit one table — one pass
            assert st["n_dist_passes"] == heads, f"{name}, {c['name']}: the sweep with bytes did not settle it? {st}"
    return stats


# ------------------------------------------------------------------ family 2: ranks that share a bitmap bit
BM = 65536
X, Y, G, H = 40000, 50001, 45000, 46000      # (bit 15 set: the upper half of the bitmap)
FILLERS = list(range(1000, 1250))
F2_MIN_COVS = (2, 9, 10)
F2_SETTINGS = {
    "default": {},
    "filter_once_0": dict(dist_filter_once=0),
    "filter_once_1": dict(dist_filter_once=1),
    "no_groups": dict(dist_groups=0),
    "small_table": dict(dist_slots=256, dist_block=64),      # the table splits: entries of the other partitions get an empty bitmap word
    "small_table_hot3": dict(dist_slots=256, dist_block=64, dist_hot_cap=3),
}


def alias_case(min_cov, several):
    """Partners of the first k-mer 0: the eight ranks X + 65536 j with the counts min_cov - 1, min_cov, min_cov + 1 in turn (a selected
    rank's alias is below min_cov and the other way round), at distance 2 or (several) at the distances 1 + j // 3; Y selected, and
    Y + 65536 with the count 1 at three distances; 250 partners more, selected, that a 256-unit table cannot hold in one partition.
    The first k-mers 1 and 2 share the first unit of one read (one group): (1, G) is selected while (2, G + 65536) is one short, and
    (2, H + 65536) is selected while (1, H) is one short."""
    def make():
        m = min_cov
        pairs = [(0, X + BM * j, 1 + j // 3 if several else 2, (m - 1, m, m + 1)[j % 3]) for j in range(8)]
        pairs += [(0, Y, 2, m)] + [(0, Y + BM, d, 1) for d in (1, 2, 3)]
        reads = cc.count_reads(pairs) + [[[0], [], FILLERS]] * m
        pairs += [(0, f, 2, m) for f in FILLERS]
        reads += [[[1, 2], [G]]] + cc.count_reads([(1, G, 1, m - 1), (2, G + BM, 1, m - 1), (2, H + BM, 1, m), (1, H, 1, m - 1)])
        pairs += [(1, G, 1, m), (2, G, 1, 1), (2, G + BM, 1, m - 1), (2, H + BM, 1, m), (1, H, 1, m - 1)]
        return dict(name=f"bitmap aliases at {'several distances' if several else 'one distance'}", clouds=cc.build(reads), pairs=pairs, min_d=1, max_d=4)
    return _case(("alias", min_cov, several), make)


def run_aliases(engine, min_cov, several, settings=F2_SETTINGS):
    c = alias_case(min_cov, several)
    below = {b for _, b, _, cnt in c["pairs"] if cnt < min_cov}
    assert all((b + BM in below or b - BM in below) for a, b, _, cnt in c["pairs"] if cnt >= min_cov and b not in FILLERS), "every selected rank has an alias that is not"
    for name, knobs in settings.items():
        st = _run(engine, c, min_cov, knobs)
        if knobs.get("dist_slots") == 256:
            assert st["n_spilled"] > 0, f"{name}: {len(FILLERS)} marked partners in one partition of a 256-unit table? {st}"


def region_case(min_cov, n, k):
    """The region layouts key the sketch and the bitmap by the rank's low 24 bits: the victim 5 and the burst 5 + 2^24, at one distance
    under the first k-mer 0, share their counter whatever the hash is.  (A set of 2^24 + 6 k-mers: on a device only.)"""
    def make():
        reads = cc.count_reads([(0, 5, 1, k)]) + [[[0], [5 + (1 << 24)] * n]] + cc.count_reads([(0, 5, 1, min_cov - k)])
        return dict(name=f"victim and burst of {n}, 2^24 ranks apart", clouds=cc.build(reads), pairs=[(0, 5, 1, min_cov), (0, 5 + (1 << 24), 1, n)], min_d=1, max_d=4)
    return _case(("region", min_cov, n, k), make)


def run_region_collision(engine, min_cov, n, k):
    for knobs in (dict(dist_regions=2, dist_block=64), dict(dist_regions=2, dist_region_bytes=1, dist_block=64), dict(dist_block=64)):
        cc.run(engine, region_case(min_cov, n, k), min_cov, knobs)      # (no refusal accepted: ranks past 2^24 are what regions are for)


# ------------------------------------------------------------------ family 3: a partner that cannot be split away
F3_MIN_D, F3_MAX_D = 16, 255
F3_DS = (16, 128, 160, 176, 192, 224, 240)      # distinct distances of ONE pair, from well below a 256-unit table to above what it may hold
F3_MIN_COV = 4
F3_LAYOUTS = {"default": {}, "narrow": dict(dist_groups=0), "wide": dict(dist_wide=1)}
SMALL = dict(dist_slots=256, dist_block=64)


def unsplittable_case(D):
    """The pair (0, 1) at the D distances 16 .. 15 + D, once each, and c = 4 (D - 1) - 2 times more at distance 16: its keys fill D slots
    of ONE partition, however far the table is split.  c is such that 5 c < 4 total with every key counted and 5 c >= 4 total with a
    single key lost (memberfiltercheck.keys): the edge (16, 0, 1) must not be there, and a table that lost a key makes it.  The pair
    (2, 3) at distance 16, F3_MIN_COV times, is the edge that the case selects.
    (The distances come sixteen to a read — 0 in unit 0, 1 in sixteen units in a row; 1 against 1 is less than min_d apart and counts
    nowhere — not one read each: the oracle walks a read's unit pairs in Python, (units)^2 / 2 steps per read.)"""
    def make():
        assert D % 16 == 0 and 16 + D - 1 <= F3_MAX_D
        c = 4 * (D - 1) - 2
        assert 5 * c < 4 * (c + D - 1) and 5 * c >= 4 * (c + D - 2) and c >= F3_MIN_COV
        reads = [[[0]] + [[] for _ in range(w - 1)] + [[1]] * 16 for w in range(16, 16 + D, 16)]
        reads += cc.count_reads([(0, 1, 16, c - 1), (2, 3, 16, F3_MIN_COV)])
        return dict(name=f"one partner at {D} distances", clouds=cc.build(reads), min_d=F3_MIN_D, max_d=F3_MAX_D, D=D, c=c)
    c = _case(("unsplittable", D), make)
    a, b, d, cnt, _ = c["hist"]
    rows = {(int(a_), int(b_), int(d_)): int(n_) for a_, b_, d_, n_ in zip(a, b, d, cnt)}
    assert rows == {**{(0, 1, 16 + i): 1 for i in range(1, D)}, (0, 1, 16): c["c"], (2, 3, 16): F3_MIN_COV}, "the oracle's histogram is the one described"
    return c


def run_unsplittable(engine, layout, sketch):
    """For every D the launch equals the oracle or is refused with -34, 'could not be partitioned far enough' — never a wrong result;
    once a D is refused every larger one is; the smallest D runs and the largest is refused.  What the refused launch leaves behind is
    what include/cfhip.h says (countcheck.refused: nothing — no counter, no edge row, the same bytes owned after a second refusal — and
    a launch that fits runs straight after)."""
    knobs = dict(F3_LAYOUTS[layout], **SMALL, dist_sketch=sketch)
    outcome = {}
    for D in F3_DS:
        c = unsplittable_case(D)
        try:
            with engine.knobs(**knobs):
                edges = pathcheck.check_clouds(engine, *c["clouds"], c["min_d"], c["max_d"], F3_MIN_COV, cc.THR, hist=c["hist"])
                st = engine.stats()
            assert edges.tolist() == [[16, 2, 3, F3_MIN_COV]] and st["n_edges"] == 1, f"{c['name']}: the oracle selects (2, 3) alone"
            outcome[D] = True
        except DeviceError as e:
            assert re.search(REFUSED_SPLIT, str(e)), f"{c['name']} {knobs}: {e}"
            outcome[D] = False
    ran = [D for D in F3_DS if outcome[D]]
    assert outcome[F3_DS[0]] and not outcome[F3_DS[-1]], f"{layout}, sketch {sketch}: {outcome}"
    assert ran == list(F3_DS[:len(ran)]), f"{layout}, sketch {sketch}: a D runs above one that is refused: {outcome}"
    first_refused = F3_DS[len(ran)]
    cc.refused(engine, dict(unsplittable_case(first_refused), pairs=[]), F3_MIN_COV, knobs, REFUSED_SPLIT, after_kernel=True)
    # ... and the same refusal straight after a launch of the SAME loaded clouds that fits (the default table): nothing of either launch
    # may be taken for edges — the refused one's rows already lie in the edge buffer when the kernel reports the failure
    c = unsplittable_case(first_refused)
    pathcheck.check_clouds(engine, *c["clouds"], c["min_d"], c["max_d"], F3_MIN_COV, cc.THR, hist=c["hist"])
    assert engine.stats()["n_edges_stored"] == 1 and engine.edges(8).any()
    with engine.knobs(**knobs):
        with pytest.raises(DeviceError, match=REFUSED_SPLIT):
            engine.dist_edges(0, c["clouds"][0].size - 1, c["min_d"], c["max_d"], F3_MIN_COV, cc.THR, 0, 1, edge_cap=9)
    st = engine.stats()
    assert [st[k] for k in ("n_emissions", "n_edges", "n_dist_passes", "n_spilled", "n_edges_stored")] == [0] * 5, st
    assert not engine.edges(8).any(), "rows handed out as edges after a launch that failed"
    return outcome

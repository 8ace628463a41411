"""The distance stage where a pair's COUNT meets a border: min_cov (which decides the counting sketch: off below 2 and above 200, 4-bit
counters up to 9, bytes from 10), the ranges of those counters (15, 255), and the width of the exact table's count field (15 bits in the
6-byte slots and next to the 16-bit distance, chosen by the host from the longest posting list: 32767 / 32768).

Every case is hand-built clouds (cf_set_clouds) whose counts are known by construction, goes through pathcheck.check_clouds — the
oracle's histogram and filter are the reference, never the code under test — and SELECTS edges: the case asserts that from the
oracle's return value, pair by pair, before it says anything about the device (the random clouds of pathcheck.check_synthetic_clouds
drive counts past 15 and 255 too, but select nothing: a fall-back that lost marks, partitions or counts would pass there).
Used by test_emu_dist_counts.py (host emulator) and test_gpu_dist_counts.py (MI355X)."""
import numpy as np
import pytest

import pathcheck
from centroflye_amd.engine import DeviceError

THR = 0.8

# the knob settings every count border is run under: the table layouts, and the launch with a part of the sketch / set-up taken out
SETTINGS = {
    "default": {},
    "wide": dict(dist_wide=1),
    "regions26": dict(dist_regions=2),
    "region_bytes": dict(dist_regions=2, dist_region_bytes=1),
    "no_sketch": dict(dist_sketch=0),
    "no_groups": dict(dist_groups=0),
    "no_classes": dict(dist_classes=0),
    "sketch_bytes": dict(dist_sketch_bits=8),
}
# a table of 256 8-byte units under one wave: passes fill up and split, "every b marked" sets up several partitions (est_limit is a few
# hundred pairs), and with a hot list of 3 the filter runs inside the bucket scan
PRESSURE = {
    "small_table": dict(dist_slots=256, dist_block=64),
    "small_table_no_sketch": dict(dist_slots=256, dist_block=64, dist_sketch=0),
    "small_table_hot3": dict(dist_slots=256, dist_block=64, dist_hot_cap=3),
}

MIN_COVS = (1, 2, 9, 10, 12, 13, 15, 16, 17, 200, 201, 255, 256, 257)      # either side of: sketch on (2), bytes (10), the guard (12), 15, off (201), 255
RANGE_COUNTS = (11, 12, 13, 14, 15, 16, 17, 254, 255, 256, 257, 300, 511, 512, 513)
RANGE_MIN_COVS = (2, 4, 9, 10, 200)
BURSTS = (11, 12, 13, 15, 16, 17, 32, 255, 256, 257)
BURST_MIN_COVS = (2, 9, 10)
POSTINGS = (32766, 32767, 32768, 32769)      # either side of the 15-bit count fields
LONG_READ = 300                              # units of the read that makes the launch take the 16-bit distance field (d up to 299 > 255)
REFUSED_REGIONS = r"\(-22\).*dist_regions does not fit this input"
REFUSED_WIDE16 = r"\(-34\).*distances above 255 with a k-mer of more than 32767 postings"


# ------------------------------------------------------------------ builders
def build(reads):
    """reads: a list of reads, each a list of cloud rows (lists of ranks, taken as they are: a row may hold a rank more than once).
    Returns (unit_ptr, cloud_ptr, entries, n_kmers) for pathcheck.check_clouds."""
    unit_ptr, cloud_ptr, entries = [0], [0], []
    for rd in reads:
        for row in rd:
            entries += row
            cloud_ptr.append(len(entries))
        unit_ptr.append(unit_ptr[-1] + len(rd))
    return np.array(unit_ptr, np.int64), np.array(cloud_ptr, np.int64), np.array(entries, np.int32), max(entries) + 1


def count_reads(pairs):
    reads = []
    for a, b, d, cnt in pairs:
        assert d >= 1 and a != b
        reads += [[[a]] + [[] for _ in range(d - 1)] + [[b]]] * cnt
    return reads


def count_clouds(pairs):
    """pairs: (a, b, d, cnt).  Each pair is cnt reads of d + 1 units — a in the first unit's cloud, b in the last one's, the units between
    empty (the construction of pathcheck.tie_clouds) — so cnt(a, b, d) is exactly cnt, whatever else the case holds."""
    return build(count_reads(pairs))


_cases = {}


def _case(key, make):
    """One set of clouds with the oracle's histogram of it, computed once and shared by every launch of the case."""
    if key not in _cases:
        c = make()
        if "hist" not in c:
            c["hist"] = pathcheck.clouds_histogram(*c["clouds"], c["min_d"], c["max_d"])
        _cases[key] = c
    return _cases[key]


def around_case(min_cov):
    """Separate first k-mers whose only pair has the count min_cov - 1, min_cov, min_cov + 1 (distances 1, 2, 3), and one first k-mer with
    three partners at distance 2 that carry those three counts."""
    def make():
        m, pairs = min_cov, []
        for i, cnt in enumerate((m - 1, m, m + 1)):
            pairs.append((2 * i, 2 * i + 1, 1 + i, cnt))
        pairs += [(6, 7 + i, 2, cnt) for i, cnt in enumerate((m - 1, m, m + 1))]
        pairs = [p for p in pairs if p[3] > 0]
        return dict(name=f"counts around min_cov {m}", clouds=count_clouds(pairs), pairs=pairs, min_d=1, max_d=4)
    return _case(("around", min_cov), make)


def range_case():
    """Every count of RANGE_COUNTS twice: as the only pair of a first k-mer of its own (count_clouds), and as one of the partners (distance
    2) of ONE first k-mer, whose counters and table hold all of them at once: read j of that k-mer holds, two units on, every partner
    whose count is above j — max(RANGE_COUNTS) postings, not their sum (the set-up of a launch without groups takes (postings)^2 steps)."""
    def make():
        n = len(RANGE_COUNTS)
        own = [(2 * i, 2 * i + 1, 1 + i % 3, cnt) for i, cnt in enumerate(RANGE_COUNTS)]
        shared = [(2 * n, 2 * n + 1 + i, 2, cnt) for i, cnt in enumerate(RANGE_COUNTS)]
        reads = count_reads(own) + [[[2 * n], [], [b for _, b, _, cnt in shared if cnt > j]] for j in range(max(RANGE_COUNTS))]
        return dict(name="counts past the counters' ranges", clouds=build(reads), pairs=own + shared, min_d=1, max_d=4)
    return _case(("range",), make)


def burst_case(n, min_cov):
    """ONE posting of the first k-mer 0 whose partner unit holds rank 1 n times — n adds to one sketch counter out of one item, four per
    lane — and min_cov reads that give the pair (0, 2) at distance 2 the count min_cov exactly."""
    def make():
        reads = [[[0], [1] * n]] + count_reads([(0, 2, 2, min_cov)])
        return dict(name=f"burst of {n} at min_cov {min_cov}", clouds=build(reads), pairs=[(0, 1, 1, n), (0, 2, 2, min_cov)], min_d=1, max_d=4)
    return _case(("burst", n, min_cov), make)


def postings_case(n, long_read=False, closed_form=True):
    """n reads of two units, rank 0 in the first and rank 1 in the second: posting lists of n entries and the pair (0, 1) at distance 1
    with the count n.  long_read: one more read of LONG_READ units, rank 2 in its first unit and rank 3 in its last, and max_d =
    LONG_READ — distances above 255 can occur and the launch takes the 16-bit distance field.
    closed_form: the histogram is written down, not computed (test_*_dist_counts compare the two at n = 300): the rows (0, 1, 1, n) and
    (2, 3, LONG_READ - 1, 1), one emission per read."""
    def make():
        unit_ptr = np.arange(n + 1, dtype=np.int64) * 2
        cloud_ptr = np.arange(2 * n + 1, dtype=np.int64)
        entries = np.tile(np.array([0, 1], np.int32), n)
        if long_read:
            unit_ptr = np.append(unit_ptr, 2 * n + LONG_READ)
            cloud_ptr = np.concatenate([cloud_ptr, np.full(LONG_READ - 1, 2 * n + 1, np.int64), [2 * n + 2]])
            entries = np.append(entries, np.array([2, 3], np.int32))
        c = dict(name=f"{n} postings" + (" and a read of %d units" % LONG_READ if long_read else ""), clouds=(unit_ptr, cloud_ptr, entries, 4 if long_read else 2),
                 pairs=[(0, 1, 1, n)], min_d=1, max_d=LONG_READ if long_read else 150)
        if closed_form:
            rows = [(0, 1, 1, n)] + ([(2, 3, LONG_READ - 1, 1)] if long_read else [])
            c["hist"] = tuple(np.array(col, np.int64) for col in zip(*rows)) + (n + bool(long_read),)
        return c
    return _case(("postings", n, long_read, closed_form), make)


def check_closed_form(n=300):
    """The histogram that postings_case writes down is the oracle's."""
    for long_read in (False, True):
        want, got = postings_case(n, long_read, closed_form=False)["hist"], postings_case(n, long_read)["hist"]
        assert all(np.array_equal(w, g) for w, g in zip(want[:4], got[:4])) and want[4] == got[4], (n, long_read)


# ------------------------------------------------------------------ the device against the oracle
def run(engine, c, min_cov, knobs=None):
    """One launch of the case under `knobs`: check_clouds compares the device with the oracle; then, from the oracle's rows, every pair the
    case planted — each is alone at its (a, b), so its share of the total is 1 — is selected with its exact count when that reaches
    min_cov and is not selected when it is short of it, and the case selects at least one edge.  Returns the stats of the launch."""
    what = f"{c['name']}, min_cov {min_cov}, {knobs or {}}"
    with engine.knobs(**(knobs or {})):
        edges = pathcheck.check_clouds(engine, *c["clouds"], c["min_d"], c["max_d"], min_cov, THR, hist=c["hist"])
        st = engine.stats()
    got = {(int(a), int(b), int(d)): int(n) for d, a, b, n in edges}
    assert got, f"{what}: the case selects no edge"
    for a, b, d, cnt in c["pairs"]:
        assert got.get((a, b, d)) == (cnt if cnt >= min_cov else None), f"{what}: pair {(a, b, d)} with the count {cnt}"
    assert len(got) == sum(1 for p in c["pairs"] if p[3] >= min_cov) == st["n_edges"], what
    return st


def run_around(engine, min_cov, settings=SETTINGS):
    c = around_case(min_cov)
    assert sorted({p[3] for p in c["pairs"]}) == [n for n in (min_cov - 1, min_cov, min_cov + 1) if n > 0]
    for knobs in settings.values():
        run(engine, c, min_cov, knobs)


def run_range(engine, min_cov, settings=SETTINGS, extra=None):
    c = range_case()
    assert min(RANGE_COUNTS) > 10 and sorted(p[3] for p in c["pairs"]) == sorted(2 * RANGE_COUNTS)
    heads = len(RANGE_COUNTS) + 1      # first k-mers with a partner unit: one table pass each, unless a table is partitioned
    stats = {}
    for name, knobs in settings.items():
        knobs = dict(knobs, **(extra or {}))
        st = stats[name] = run(engine, c, min_cov, knobs)
        # Which path ran, from the passes (cf_stats names no path).  With bytes for counters the 256th add of a pair sees 255, whatever
        # the order of the adds: the first k-mer goes to "every b marked", and under a table of 256 units that path sets up several
        # partitions for the k-mers with hundreds of pairs — more passes than first k-mers although no table filled up and split.
        # The same without the sketch; 4-bit counters stop at their guard and need not wrap.
        sketch = knobs.get("dist_sketch", 1) and 2 <= min_cov <= 200
        in_bytes = sketch and (min_cov >= 10 or knobs.get("dist_sketch_bits") == 8)
        assert st["n_dist_passes"] >= heads, (name, min_cov, st)
        if knobs.get("dist_slots") == 256 and st["n_spilled"] == 0 and (in_bytes or not sketch):
            assert st["n_dist_passes"] > heads, f"{name}, min_cov {min_cov}: every b marked, in one partition? {st}"
    return stats


def run_burst(engine, n, min_cov):
    c = burst_case(n, min_cov)
    _, cloud_ptr, entries, _ = c["clouds"]
    assert entries[cloud_ptr[1]:cloud_ptr[2]].tolist() == [1] * n and int((entries == 0).sum()) == 1 + min_cov, "one row holds the rank n times; one posting brings them all"
    for knobs in ({}, dict(dist_sketch_bits=8), dict(dist_sketch=0)):
        run(engine, c, min_cov, knobs)




def refused(engine, c, min_cov, knobs, message, after_kernel=False):
    """The launch is refused with `message`, twice: the context owns as many bytes after the second refusal as after the first, nothing is
    left of the refused launch — no counter (cf_dist_edges zeroes them when it begins), no edge row, no unique bit — and the context is
    usable: a launch that fits runs straight after.
    after_kernel: the refusal comes from the kernel itself, which has run to its end (include/cfhip.h, cf_dist_edges): the unique mask
    may hold bits of the first k-mers that did fit, and is not looked at."""
    live = []
    for _ in range(2):
        with engine.knobs(**knobs):
            with pytest.raises(DeviceError, match=message):
                pathcheck.check_clouds(engine, *c["clouds"], c["min_d"], c["max_d"], min_cov, THR, hist=c["hist"])
        st = engine.stats()
        live.append(st["hbm_bytes_live"])
        assert [st[k] for k in ("n_emissions", "n_edges", "n_dist_passes", "n_spilled", "n_edges_stored", "n_unique")] == [0] * 6, st
        assert not engine.edges(8).any() and (after_kernel or not engine.unique_mask().any()), "no edge rows and no unique bits of a refused launch"
    assert live[0] == live[1], f"hbm_bytes_live {live[0]} after the first refusal, {live[1]} after the second"
    run(engine, postings_case(300), min_cov)


# n x layout of the posting-list border.  "default", "regions" (dist_regions=2) and "wide" (dist_wide=1) run the two-unit reads alone;
# "wide16" adds the read of LONG_READ units with max_d = LONG_READ, so that the launch takes the 16-bit distance field.
POSTING_LAYOUTS = {"default": {}, "regions": dict(dist_regions=2), "wide": dict(dist_wide=1), "wide16": {}}
POSTING_REFUSALS = {"regions": REFUSED_REGIONS, "wide16": REFUSED_WIDE16}


def postings_refused(n, layout):
    return n > 32767 and layout in POSTING_REFUSALS


def postings_in_groups(n, layout):
    """The launch sweeps groups: the 6-byte layout as the launch picks it by itself.  Every other launch that runs counts
    the pairs of one k-mer's postings with itself in cf_items_count_kernel, in (postings)^2 / 16 steps per lane: 3.2 s of an MI355X at
    32768 postings (0.19 s at 8000, 0.75 s at 16000), and ten minutes of the host emulator — which therefore runs the launches in groups
    and the refusals only."""
    return n <= 32767 and layout == "default"


def run_postings(engine, n, layout, min_cov=4):
    """Posting lists of n entries and the pair (0, 1) with the count n, either side of the 15 bits that the 6-byte slots (cnt - 1) and the
    16-bit-distance slots (cnt, the selection bit directly above it) have for a count.
      up to 32767   every layout runs and equals the oracle;
      from 32768    the forced regions are refused — which proves that the default launch of the same clouds, equal to the oracle, has
                    left the 6-byte slots by itself (both 6-byte layouts ask for max_post <= 32767) — and so is the 16-bit distance
                    field; the default and the forced 8-byte slots (23 bits) run."""
    c = postings_case(n, long_read=layout == "wide16")
    if postings_refused(n, layout):
        refused(engine, c, min_cov, POSTING_LAYOUTS[layout], POSTING_REFUSALS[layout])
    else:
        run(engine, c, min_cov, POSTING_LAYOUTS[layout])

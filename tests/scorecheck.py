"""The exact scorer of a frozen cloud contig, restated on sorted numpy arrays, and the case bodies shared by the emulator and the
GPU suite (test_emu_score_reads.py, test_gpu_score_reads.py).

The reference: scripts/cloud_contig.py:26-41 (CloudContig.add_read), :46-76 (calc_inters_score), :78-84 (get_spread_kmers),
:98-114 (map_reads).  On the cloud CSR (unit_ptr per read, cloud_ptr per unit, entries = k-mer ranks):
  contig   count[(p, x)] = backbone reads whose unit i holds x with pos + i == p; F = the pairs (x, p) with count >= max(1, f)
           (freq_clouds: frequent AT p); max_pos = the largest covered position (0 for an empty contig).
  score    of read r at start s: every (unit i, k-mer x of it) with (x, s + i) in F is one hit; s0 = units with a hit, s1 = hits.
           A pair of F lies at p <= max_pos, which is all the truncation `i < max_pos - s + 1` says.
  answer   calc_inters_score(r, lo, hi, t0, t1): among lo <= s <= hi with s0 >= t0 and s1 >= t1 the maximum of (s0, s1, s); a start
           without a hit scores (0, 0), so with t0 <= 0 and t1 <= 0 and no hit anywhere the answer is hi.  (-1, 0, 0) is None.
  verdict  map_reads(threshold): the answer over [0, max_pos - n + 1] under (2, 10), kept iff pos == 0 or (s0, s1) > threshold.
  spread   the frequent ranks with more than max_npos positions of ANY count.
Everything is sorting, searching and counting on flat arrays; it shares no code with the kernels or with
centroflye_amd/cloud_contig.py.  `wrong` plants one of seven plausible misreadings of the reference, so that the goldens can show
that they tell each of them apart (tests/golden/make_golden_score_reads.py records how many cases each one changes).
All comparisons are integer-exact."""
import json
import os

import numpy as np

from mapcheck import DEFAULT_WINDOW, _ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "score_reads_cases.json")
MAP_GOLDEN = os.path.join(ROOT, "tests", "golden", "map_reads_cases.json")
WRONG_RULES = ("frequent_elsewhere_counts", "p_for_max_pos", "smaller_start_on_ties", "overhang_refused", "keep_on_equal",
               "no_start_zero_rule", "inner_is_the_callers_threshold")
SPREAD_MAX_NPOS = (0, 1, 5)
STRIDE_CASE = "hand_gap_b"      # check_past_the_launch_cap: the hand-built source (no pipeline run), max_pos 57, 18 reads
INNER = (2, 10)      # calc_inters_score's defaults, which map_reads does not override (cloud_contig.py:48, :105-106)


def contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, f):
    unit_ptr, cloud_ptr, entries = (np.asarray(a, np.int64) for a in (unit_ptr, cloud_ptr, entries))
    b_reads, b_pos = np.asarray(b_reads, np.int64).reshape(-1), np.asarray(b_pos, np.int64).reshape(-1)
    f = max(1, int(f))
    units, owner = _ranges(unit_ptr[b_reads], unit_ptr[b_reads + 1])
    upos = b_pos[owner] + (units - unit_ptr[b_reads][owner])
    max_pos = int(upos.max()) if upos.size else 0
    P = int(np.unique(upos).size)
    ent, eowner = _ranges(cloud_ptr[units], cloud_ptr[units + 1])
    pair, count = np.unique((entries[ent] << 32) | upos[eowner], return_counts=True)      # sorted by (rank, position)
    rank, pos = pair >> 32, pair & 0xFFFFFFFF
    here = count >= f
    anywhere = np.isin(rank, np.unique(rank[here]))
    return dict(P=P, max_pos=max_pos, exact_rank=rank[here], exact_pos=pos[here], all_rank=rank[anywhere], all_pos=pos[anywhere],
                n_exact_pairs=int(here.sum()))


def read_hits(unit_ptr, cloud_ptr, entries, c, r, wrong=None):
    """(p, i, n): every (contig position p of F, unit i of read r) that share a k-mer, and the read's number of units."""
    unit_ptr, cloud_ptr, entries = (np.asarray(a, np.int64) for a in (unit_ptr, cloud_ptr, entries))
    u0, u1 = int(unit_ptr[r]), int(unit_ptr[r + 1])
    rows_rank, rows_pos = (c["all_rank"], c["all_pos"]) if wrong == "frequent_elsewhere_counts" else (c["exact_rank"], c["exact_pos"])
    ent, unit = _ranges(cloud_ptr[u0:u1], cloud_ptr[u0 + 1:u1 + 1])
    x = entries[ent]
    rows, owner = _ranges(np.searchsorted(rows_rank, x, "left"), np.searchsorted(rows_rank, x, "right"))
    return rows_pos[rows], unit[owner], u1 - u0


def best_start(hits, c, lo=0, hi=None, t0=2, t1=10, wrong=None):
    """(pos, s0, s1) of calc_inters_score over [lo, hi] under (t0, t1) from the hits of a read; (-1, 0, 0) for None."""
    p, i, n = hits
    end = max(c["P"] - 1, 0) if wrong == "p_for_max_pos" else c["max_pos"]
    if hi is None:
        hi = end - n + 1
    if lo > hi:
        return (-1, 0, 0)
    s = p - i
    ok = (s >= lo) & (s <= hi) & (p <= end)
    if wrong == "overhang_refused":
        ok &= s + n - 1 <= end
    s, i = s[ok], i[ok]
    starts, s1 = np.unique(s, return_counts=True)
    s0 = np.bincount(np.searchsorted(starts, np.unique((s << 32) | i) >> 32), minlength=starts.size)
    ok = (s0 >= t0) & (s1 >= t1)
    starts, s0, s1 = starts[ok], s0[ok], s1[ok]
    if not starts.size:
        if t0 <= 0 and t1 <= 0:      # every start scores (0, 0) and qualifies
            return (int(lo if wrong == "smaller_start_on_ties" else hi), 0, 0)
        return (-1, 0, 0)
    w = np.lexsort((-starts if wrong == "smaller_start_on_ties" else starts, s1, s0))[-1]
    return (int(starts[w]), int(s0[w]), int(s1[w]))


def score_read(unit_ptr, cloud_ptr, entries, c, r, lo=0, hi=None, t0=2, t1=10, wrong=None):
    """(pos, s0, s1) of calc_inters_score(read r, lo, hi, t0, t1) on the contig c; (-1, 0, 0) for None."""
    return best_start(read_hits(unit_ptr, cloud_ptr, entries, c, r, wrong), c, lo, hi, t0, t1, wrong)


def verdict(unit_ptr, cloud_ptr, entries, c, r, threshold, wrong=None):
    """map_reads' entry of read r: [1, pos, s0, s1] when it is kept, [0] when it is not."""
    inner = tuple(threshold) if wrong == "inner_is_the_callers_threshold" else INNER
    pos, s0, s1 = score_read(unit_ptr, cloud_ptr, entries, c, r, 0, None, inner[0], inner[1], wrong)
    beats = (s0, s1) >= tuple(threshold) if wrong == "keep_on_equal" else (s0, s1) > tuple(threshold)
    if (pos == 0 and wrong != "no_start_zero_rule") or beats:
        return [1, pos, s0, s1]
    return [0]


def spread(c, max_npos):
    """The ranks of get_spread_kmers(max_npos), ascending."""
    rank, npos = np.unique(c["all_rank"], return_counts=True)
    return rank[npos > max_npos]


def spread_figures(cloud_entries, c, max_npos):
    """What the golden records of a set of spread k-mers without naming them: how many, the positions they have in all, and how
    many cloud entries of ALL reads hold one."""
    rank, npos = np.unique(c["all_rank"], return_counts=True)
    sel = npos > max_npos
    return [int(sel.sum()), int(npos[sel].sum()), int(np.isin(np.asarray(cloud_entries, np.int64), rank[sel]).sum())]


def read_row(unit_ptr, cloud_ptr, entries, c, r, threshold, sub, wrong=None):
    """The golden's row of one read: full range, overhang range, sub-range [a, b], the single start c0 under (0, 0), verdict."""
    a, b, c0 = sub
    t0, t1 = threshold
    A = (unit_ptr, cloud_ptr, entries, c, r)
    end = max(c["P"] - 1, 0) if wrong == "p_for_max_pos" else c["max_pos"]
    return (list(score_read(*A, 0, None, t0, t1, wrong)) + list(score_read(*A, 0, end, t0, t1, wrong)) + [a, b]
            + list(score_read(*A, a, b, t0, t1, wrong)) + [c0] + list(score_read(*A, c0, c0, 0, 0, wrong))
            + verdict(unit_ptr, cloud_ptr, entries, c, r, threshold, wrong))


# ------------------------------------------------------------------ golden cases
def load_cases():
    """The score cases with the source, backbone and f of the map case each one is built on (`of`)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    with open(MAP_GOLDEN) as f:
        m = json.load(f)
    base = {c["name"]: c for c in m["cases"]}
    for case in g["cases"]:
        b = base[case["of"]]
        case.update(source=b["source"], backbone=b["backbone"], f=b["f"], read_ids=list(b["expect"]["reads"]),
                    fast=b["expect"]["reads"] if b["threshold"] == case["threshold"] else None)
    g["sources"] = m["sources"]
    return g


def _triples(pos, s0, s1):
    return [list(t) for t in zip(pos.tolist(), s0.tolist(), s1.tolist())]


def check_case(src, case, window=0):
    """One golden case through the C ABI against the REFERENCE's recorded rows, and the numpy statement above against the same.
    src: mapcheck.Sources.  window: map_window forced to that many slots.  Returns how many reads had their full range split
    over several windows."""
    ids, unit_ptr, cloud_ptr, entries = src.use(case["source"])
    e = src.engine
    row = {r_id: i for i, r_id in enumerate(ids)}
    b_reads = np.array([row[r] for r, _ in case["backbone"]], np.int64)
    b_pos = np.array([p for _, p in case["backbone"]], np.int64)
    t0, t1 = case["threshold"]
    tag = f"{case['name']} (window {window})"
    q = np.array([row[r] for r in case["read_ids"]], np.int64)
    want = case["reads"]
    c = contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, case["f"])
    assert c["max_pos"] == case["max_pos"] and c["n_exact_pairs"] == case["n_exact_pairs"], f"{tag}: numpy contig vs reference"
    numpy_rows = [read_row(unit_ptr, cloud_ptr, entries, c, int(r), (t0, t1), w[6:8] + [w[11]]) for r, w in zip(q, want)]
    bad = [(r, g, w) for r, g, w in zip(case["read_ids"], numpy_rows, want) if g != w]
    assert not bad, f"{tag}: {len(bad)} numpy rows differ from the reference, first {bad[:2]}"
    for m in SPREAD_MAX_NPOS:
        assert spread_figures(entries, c, m) == case["spread"][str(m)], f"{tag}: numpy spread k-mers, max_npos {m}"
    with e.knobs(map_window=window):
        e.contig_build(b_reads, b_pos, case["f"])
        info = e.contig_info()
        assert info["max_pos"] == case["max_pos"] and e.contig_exact_info()["n_exact_pairs"] == case["n_exact_pairs"], tag
        full = _triples(*e.score_reads(q, None, None, t0, t1))
        over = _triples(*e.score_reads(q, 0, case["max_pos"], t0, t1))
        a, b, c0 = (np.array([w[k] for w in want], np.int64) for k in (6, 7, 11))
        sub = _triples(*e.score_reads(q, a, b, t0, t1))
        one = _triples(*e.score_reads(q, c0, c0, 0, 0))
        inner = e.score_reads(q, None, None, *INNER)
    from centroflye_amd.read_mapper import kept_by_map_reads
    keep = kept_by_map_reads(*inner, (t0, t1))
    verdicts = [[1] + t if k else [0] for t, k in zip(_triples(*inner), keep.tolist())]
    got = [f + o + [w[6], w[7]] + s + [w[11]] + x + v for f, o, s, x, v, w in zip(full, over, sub, one, verdicts, want)]
    bad = [(r, g, w) for r, g, w in zip(case["read_ids"], got, want) if g != w]
    assert not bad, f"{tag}: {len(bad)} device rows differ from the reference, first {bad[:2]}"
    for m in SPREAD_MAX_NPOS:
        assert np.array_equal(e.contig_spread(m), spread(c, m)), f"{tag}: device spread k-mers, max_npos {m}"
    n_units = (np.asarray(unit_ptr)[q + 1] - np.asarray(unit_ptr)[q])
    return int(((case["max_pos"] - n_units + 1 - 0 + 1) > (window or DEFAULT_WINDOW)).sum())


# ------------------------------------------------------------------ a hand-built CSR at the kernel's shape borders
def synthetic_contig(seed=11, n_pos=5000, n_reads=300, n_backbone=250, K=40000):
    """Reads cut from an array of n_pos positions (more than the default window of 2 048 starts): position p holds 0 - 150 ranks
    (units of more than 64 entries: several strides of a wave), among them four ranks that recur with periods 5, 7, 7 and 11
    (rows of hundreds of positions, and ties between starts one period apart).  A read is a window of 1 - 120 positions that keeps
    each rank with probability 0.85; the first n_backbone reads, laid where they were cut, are the backbone.
    Returns (spec for mapcheck.install_synthetic, backbone reads, backbone positions, the start every read was cut at)."""
    rng = np.random.default_rng(seed)
    recurring = [(K - 1 - j, period) for j, period in enumerate((5, 7, 7, 11))]
    content = []
    for p in range(n_pos):
        own = rng.choice(K - 4, size=int(rng.integers(0, 147)), replace=False)
        content.append(np.concatenate([own, [x for x, period in recurring if p % period == x % period]]).astype(np.int64))
    unit_ptr, cloud_ptr, entries, cut = [0], [0], [], []
    for r in range(n_reads):
        n = int(rng.integers(1, 121))
        p0 = int(rng.integers(0, n_pos - n + 1))
        cut.append(p0)
        for i in range(n):
            u = content[p0 + i]
            u = np.sort(u[rng.random(u.size) < 0.85])
            entries.append(u)
            cloud_ptr.append(cloud_ptr[-1] + u.size)
        unit_ptr.append(len(cloud_ptr) - 1)
    spec = dict(unit_ptr=unit_ptr, cloud_ptr=cloud_ptr, entries=np.concatenate(entries).astype(np.int32), K=K)
    return spec, np.arange(n_backbone, dtype=np.int64), np.array(cut[:n_backbone], np.int64), np.array(cut, np.int64)


_SYNTHETIC = {}


def synthetic_reference(f=2):
    """The synthetic contig and the numpy statement's answers for the queries of check_synthetic, computed once."""
    if f in _SYNTHETIC:
        return _SYNTHETIC[f]
    spec, b_reads, b_pos, cut = synthetic_contig()
    unit_ptr, cloud_ptr, entries = (np.asarray(spec[k], np.int64) for k in ("unit_ptr", "cloud_ptr", "entries"))
    R = unit_ptr.size - 1
    c = contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, f)
    A = (unit_ptr, cloud_ptr, entries, c)
    assert c["max_pos"] > 2 * DEFAULT_WINDOW and int(np.diff(cloud_ptr).max()) > 64
    rng = np.random.default_rng(3)
    lo = rng.integers(0, c["max_pos"] - 2500, R)
    hi = lo + rng.integers(0, 2500, R)                       # sub-ranges up to more than a window wide
    hits = [read_hits(*A, r) for r in range(R)]
    ref = dict(spec=spec, b_reads=b_reads, b_pos=b_pos, cut=cut, c=c, R=R, lo=lo, hi=hi, q=rng.permutation(R)[:50], f=f,
               full=[list(best_start(hits[r], c, 0, None, 2, 10)) for r in range(R)],
               over=[list(best_start(hits[r], c, 0, c["max_pos"], 0, 0)) for r in range(R)],
               sub=[list(best_start(hits[r], c, int(lo[r]), int(hi[r]), 1, 1)) for r in range(R)],
               at_cut=[list(best_start(hits[r], c, int(cut[r]), int(cut[r]), 0, 0)) for r in range(R)],
               spread={m: spread(c, m) for m in (0, 1, 5, 600, 10 ** 6)}, entries=int(entries.size))
    _SYNTHETIC[f] = ref
    return ref


def check_synthetic(engine, window=0):
    """The synthetic contig through the C ABI against the numpy statement: full ranges, overhang ranges, sub-ranges wider than
    a window, ranges of one start, and one start rescored against what the full-range pass gave it.  Returns figures of the run."""
    import mapcheck
    ref = synthetic_reference()
    mapcheck.install_synthetic(engine, ref["spec"])
    c, R, lo, hi, cut, q = (ref[k] for k in ("c", "R", "lo", "hi", "cut", "q"))
    with engine.knobs(map_window=window):
        engine.contig_build(ref["b_reads"], ref["b_pos"], ref["f"])
        assert engine.contig_info()["max_pos"] == c["max_pos"] and engine.contig_exact_info()["n_exact_pairs"] == c["n_exact_pairs"]
        full = _triples(*engine.score_reads(None, None, None, 2, 10))
        over = _triples(*engine.score_reads(None, 0, c["max_pos"], 0, 0))
        sub = _triples(*engine.score_reads(None, lo, hi, 1, 1))
        at_cut = _triples(*engine.score_reads(None, cut, cut, 0, 0))
        won = np.array([max(t[0], 0) for t in full], np.int64)
        at_won = _triples(*engine.score_reads(None, won, won, 0, 0))
        some = _triples(*engine.score_reads(q, lo[q], hi[q], 1, 1))
        spreads = {m: engine.contig_spread(m) for m in ref["spread"]}
    assert full == ref["full"], "full ranges"
    assert over == ref["over"], "overhang ranges"
    assert sub == ref["sub"], "sub-ranges"
    assert at_cut == ref["at_cut"], "ranges of one start"
    assert some == [sub[int(r)] for r in q], "queries as a subset"
    # a range of one start at s gives the score the full-range pass gave s
    placed = [r for r in range(R) if full[r][0] >= 0]
    assert all(at_won[r] == full[r] for r in placed), "one start against the full range"
    for m, got in spreads.items():
        assert np.array_equal(got, ref["spread"][m]) and got.dtype == np.int32, f"spread k-mers, max_npos {m}"
    assert spreads[600].size >= 3 and spreads[10 ** 6].size == 0 and spreads[0].size > spreads[5].size > spreads[600].size
    return dict(reads=R, entries=ref["entries"], max_pos=c["max_pos"], n_exact_pairs=c["n_exact_pairs"], mapped=len(placed),
                mapped_where_cut=sum(1 for r in placed if full[r][0] == cut[r]),
                mapped_elsewhere=sum(1 for r in placed if full[r][0] != cut[r]))


# ------------------------------------------------------------------ more queries than launched workgroups
def stride_queries(case, unit_ptr, row, n_cu, seed=192):
    """192 x n_cu + 5 queries for a golden case: its reads repeated in a seeded shuffle, each with one of its three recorded ranges
    (the full range, the overhang range, the sub-range), so that every workgroup of the 64 x n_cu launched takes three queries and
    some a fourth.  Queries one launch stride apart run in the same workgroup, one after the other on the same LDS window: they are
    drawn to differ in read and in range.  Returns (reads, lo, hi, the recorded (pos, s0, s1) per query, the stride)."""
    rng = np.random.default_rng(seed)
    stride = 64 * n_cu
    n = 192 * n_cu + 5
    ids = [row[r] for r in case["read_ids"]]
    q, lo, hi, want = [], [], [], []
    for i in range(n):
        while True:
            j, kind = int(rng.integers(0, len(ids))), int(rng.integers(0, 3))
            w = case["reads"][j]
            r = ids[j]
            n_units = int(unit_ptr[r + 1] - unit_ptr[r])
            a, b = ((0, case["max_pos"] - n_units + 1), (0, case["max_pos"]), (w[6], w[7]))[kind]
            if i < stride or (q[i - stride] != r and (lo[i - stride], hi[i - stride]) != (a, b)):
                break
        q.append(r), lo.append(a), hi.append(b), want.append(w[(0, 3, 8)[kind]:(3, 6, 11)[kind]])
    return np.array(q, np.int64), np.array(lo, np.int64), np.array(hi, np.int64), want, stride


def check_past_the_launch_cap(src, case):
    """One golden case as 192 x n_cu + 5 queries in one call, three times what the launch has workgroups, against the REFERENCE's
    recorded rows gathered by query, with map_window forced to 3 (a range takes many windows) and left at its default (one window
    per range).  Returns figures of the run."""
    ids, unit_ptr, cloud_ptr, entries = src.use(case["source"])
    e = src.engine
    n_cu = e.device_info()["n_cu"]
    row = {r_id: i for i, r_id in enumerate(ids)}
    q, lo, hi, want, stride = stride_queries(case, np.asarray(unit_ptr), row, n_cu)
    n = q.size
    assert n == 192 * n_cu + 5 and n > 3 * stride
    # neighbours in a workgroup's stride differ in read and in range, and the recorded answers are not all alike
    assert (q[stride:] != q[:-stride]).all() and ((lo[stride:] != lo[:-stride]) | (hi[stride:] != hi[:-stride])).all()
    placed = sum(w[0] >= 0 for w in want)
    assert len({tuple(w) for w in want}) >= 10 and 4 * placed >= n and 8 * (n - placed) >= n
    assert int((hi - lo).max()) >= 3 * 3      # a range of several windows of 3 starts
    t0, t1 = case["threshold"]
    e.contig_build([row[r] for r, _ in case["backbone"]], [p for _, p in case["backbone"]], case["f"])
    assert e.contig_info()["max_pos"] == case["max_pos"]
    for window in (3, 0):
        with e.knobs(map_window=window):
            got = _triples(*e.score_reads(q, lo, hi, t0, t1))
            bad = [i for i in range(n) if got[i] != want[i]]
            assert not bad, (f"{case['name']} (window {window}): {len(bad)} of {n} queries differ from the reference, first at query {bad[0]} "
                             f"(the {bad[0] // stride + 1}. of its workgroup): {got[bad[0]]} for {want[bad[0]]}")
    return dict(n_cu=n_cu, queries=n, workgroups=stride, placed=placed, distinct_answers=len({tuple(w) for w in want}))

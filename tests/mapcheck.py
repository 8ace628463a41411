"""Mapping of reads onto a frozen cloud contig, restated on numpy arrays, and the case bodies shared by the emulator and the
GPU suite (test_emu_map_reads.py, test_gpu_map_reads.py).

The reference: scripts/cloud_contig.py:26-41 (CloudContig.add_read for every backbone read) and :87-95, :117-156
(map_reads_fast).  On the cloud CSR (unit_ptr per read, cloud_ptr per unit, entries = k-mer ranks):
  contig   count[(p, x)] = backbone reads whose unit i holds x with pos + i == p; x is frequent when count[(p, x)] >= max(1, f)
           somewhere; the seeds are EVERY (x, p) with count >= 1 of a frequent x; coverage counts units (an empty cloud still
           covers its position); P = distinct covered positions; max_pos = the largest one (0 for an empty contig).
  scores   every seed (x, q) and every (unit i of the read) holding x with q >= i adds one hit to start q - i of unit i.
  answer   among the starts s with s + n <= P, s0 = units with a hit >= t0 and s1 = hits >= t1: the maximum of (s0, s1, s).
Everything is sorting, searching and counting on flat arrays; it shares no code with the kernels or with
centroflye_amd/cloud_contig.py.  `wrong` plants one of five plausible misreadings of the reference, so that the goldens can
show that they tell each of them apart (tests/golden/make_golden_map_reads.py records how many cases each one changes).
All comparisons are integer-exact."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_reads_cases.json")
WRONG_RULES = ("seeds_only_where_frequent", "q_gt_i", "p_is_max_pos_plus_1", "smaller_start_on_ties", "s1_before_s0")
DEFAULT_WINDOW = 2048      # slots of the score table under map_window 0 (CF_MAP_WINDOW_DEFAULT, CF_SCORE_WINDOW_DEFAULT)


def _ranges(lo, hi):
    """Concatenation of arange(lo[j], hi[j]) and the j of every element."""
    n = (hi - lo).astype(np.int64)
    owner = np.repeat(np.arange(n.size, dtype=np.int64), n)
    first = np.cumsum(n) - n
    return lo[owner] + (np.arange(int(n.sum()), dtype=np.int64) - first[owner]), owner


def contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, f, wrong=None):
    unit_ptr, cloud_ptr, entries = (np.asarray(a, np.int64) for a in (unit_ptr, cloud_ptr, entries))
    b_reads, b_pos = np.asarray(b_reads, np.int64).reshape(-1), np.asarray(b_pos, np.int64).reshape(-1)
    f = max(1, int(f))
    units, owner = _ranges(unit_ptr[b_reads], unit_ptr[b_reads + 1])                 # every unit of every backbone read
    upos = b_pos[owner] + (units - unit_ptr[b_reads][owner])                         # and the position it is laid on
    max_pos = int(upos.max()) if upos.size else 0
    coverage = np.bincount(upos, minlength=max_pos + 1).astype(np.int32) if upos.size else np.zeros(0, np.int32)
    P = int(np.count_nonzero(coverage))
    ent, eowner = _ranges(cloud_ptr[units], cloud_ptr[units + 1])
    key = (entries[ent] << 32) | upos[eowner]
    pair, count = np.unique(key, return_counts=True)                                  # sorted by (rank, position)
    rank, pos = pair >> 32, pair & 0xFFFFFFFF
    frequent = np.unique(rank[count >= f])
    keep = np.isin(rank, frequent)
    if wrong == "seeds_only_where_frequent":
        keep = count >= f
    return dict(P=P, max_pos=max_pos, n_freq_kmers=int(frequent.size), coverage=coverage, seed_rank=rank[keep], seed_pos=pos[keep],
                n_pairs=int(np.count_nonzero(np.isin(rank, frequent))))


def map_read(unit_ptr, cloud_ptr, entries, c, r, t0, t1, wrong=None):
    """(pos, s0, s1) of read r on the contig c, pos = -1 and zeros when no start qualifies."""
    unit_ptr, cloud_ptr, entries = (np.asarray(a, np.int64) for a in (unit_ptr, cloud_ptr, entries))
    u0, u1 = int(unit_ptr[r]), int(unit_ptr[r + 1])
    n = u1 - u0
    limit = (c["max_pos"] + 1 if wrong == "p_is_max_pos_plus_1" else c["P"]) - n
    if n == 0 or limit < 0:
        return (-1, 0, 0)
    ent, unit = _ranges(cloud_ptr[u0:u1], cloud_ptr[u0 + 1:u1 + 1])                   # unit = index i of the entry's unit
    x = entries[ent]
    seeds, owner = _ranges(np.searchsorted(c["seed_rank"], x, "left"), np.searchsorted(c["seed_rank"], x, "right"))
    q, i = c["seed_pos"][seeds], unit[owner]
    ok = (q > i) if wrong == "q_gt_i" else (q >= i)
    s, i = (q - i)[ok], i[ok]
    ok = s <= limit
    s, i = s[ok], i[ok]
    if not s.size:
        return (-1, 0, 0)
    starts, s1 = np.unique(s, return_counts=True)
    s0 = np.bincount(np.searchsorted(starts, np.unique((s << 32) | i) >> 32), minlength=starts.size)
    ok = (s0 >= t0) & (s1 >= t1)
    starts, s0, s1 = starts[ok], s0[ok], s1[ok]
    if not starts.size:
        return (-1, 0, 0)
    tie = -starts if wrong == "smaller_start_on_ties" else starts
    order = np.lexsort((tie, s0, s1)) if wrong == "s1_before_s0" else np.lexsort((tie, s1, s0))
    w = order[-1]
    return (int(starts[w]), int(s0[w]), int(s1[w]))


def hit_span(unit_ptr, cloud_ptr, entries, c, r):
    """Number of admissible starts between the first and the last one of read r that have a hit (0: none): a score table of W
    slots takes ceil(span / W) passes."""
    unit_ptr, cloud_ptr, entries = (np.asarray(a, np.int64) for a in (unit_ptr, cloud_ptr, entries))
    u0, u1 = int(unit_ptr[r]), int(unit_ptr[r + 1])
    if u1 == u0 or c["P"] < u1 - u0:
        return 0
    ent, unit = _ranges(cloud_ptr[u0:u1], cloud_ptr[u0 + 1:u1 + 1])
    x = entries[ent]
    seeds, owner = _ranges(np.searchsorted(c["seed_rank"], x, "left"), np.searchsorted(c["seed_rank"], x, "right"))
    s = c["seed_pos"][seeds] - unit[owner]
    s = s[(s >= 0) & (s <= c["P"] - (u1 - u0))]
    return int(s.max() - s.min() + 1) if s.size else 0


def map_all(unit_ptr, cloud_ptr, entries, c, reads, t0, t1, wrong=None):
    return [map_read(unit_ptr, cloud_ptr, entries, c, int(r), t0, t1, wrong) for r in reads]


# ------------------------------------------------------------------ golden cases
def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)


def synthetic_arrays(spec):
    """A hand-built case carries its clouds: reads of one base per unit, ranks 0 .. K - 1 as the k-mer set."""
    unit_ptr = np.asarray(spec["unit_ptr"], np.int64)
    U = int(unit_ptr[-1])
    return dict(bases=np.full(U, ord("A"), np.uint8), read_off=unit_ptr, unit_ptr=unit_ptr, unit_start=np.arange(U, dtype=np.int64),
                unit_end=np.arange(U, dtype=np.int64) + 1, cloud_ptr=np.asarray(spec["cloud_ptr"], np.int64),
                entries=np.asarray(spec["entries"], np.int32), K=int(spec["K"]))


def install_synthetic(engine, spec):
    a = synthetic_arrays(spec)
    engine.load_arrays(a["bases"], a["read_off"], a["unit_ptr"], a["unit_start"], a["unit_end"])
    engine.set_kmers(np.arange(a["K"], dtype=np.uint64), 16)
    engine.set_clouds(a["cloud_ptr"], a["entries"])
    return [str(i) for i in range(a["unit_ptr"].size - 1)], a["unit_ptr"], a["cloud_ptr"], a["entries"]


class Sources:
    """The clouds of each golden source, installed on the engine on demand (one source resident at a time).  A source is a
    fixture report with the reference's own genomic k-mers (through the package's drop-in modules, as scripts/map_reads.py
    does it) or a hand-built CSR."""

    def __init__(self, engine, report_of, cases):
        self.engine, self.report_of, self.sources = engine, report_of, cases["sources"]
        self.current, self.state = None, None

    def use(self, name):
        if self.current == name:
            return self.state
        spec = self.sources[name]
        if spec["kind"] == "synthetic":
            from centroflye_amd import session
            session._loaded = None      # (the session's engine now holds other reads)
            self.state = install_synthetic(self.engine, spec)
        else:
            import types
            from centroflye_amd import read_mapper, session
            assert session._engine is self.engine
            kfile = os.path.join(ROOT, "tests", "golden", spec["kmers_file"])
            params = types.SimpleNamespace(ncrf=self.report_of(spec["fixture"]), genomic_kmers=kfile, read_placement=os.devnull,
                                           outdir=os.path.join(os.path.dirname(self.report_of(spec["fixture"])), "map_out"),
                                           n_motif=spec["n_motif"], k_cloud=spec["k_cloud"], min_kmer_mult=spec["min_kmer_mult"])
            clouds = read_mapper.ReadMapper(params).clouds()
            assert clouds.on_device() is self.engine
            self.state = (list(clouds.report.packed.ids), np.asarray(clouds.unit_ptr, np.int64), np.asarray(clouds.cloud_ptr, np.int64),
                          np.asarray(clouds.entries, np.int64))
        self.current = name
        return self.state


def check_case(src, case, window=0, log=None):
    """One golden case through the C ABI: the contig's figures and coverage and (pos, s0, s1) of every query read against the
    REFERENCE's recorded answers, and the numpy statement above against the same (so that it may stand in at sizes the reference
    cannot run).  window: map_window forced to that many slots.  Returns cf_contig_info's figures and, under
    "multi_window_reads", how many query reads have hits spread over more starts than one window holds."""
    ids, unit_ptr, cloud_ptr, entries = src.use(case["source"])
    e = src.engine
    row = {r_id: i for i, r_id in enumerate(ids)}
    b_reads = np.array([row[r] for r, _ in case["backbone"]], np.int64)
    b_pos = np.array([p for _, p in case["backbone"]], np.int64)
    want = case["expect"]
    t0, t1 = case["threshold"]
    query = [row[r] for r in want["reads"]]
    with e.knobs(map_window=window):
        e.contig_build(b_reads, b_pos, case["f"])
        info = e.contig_info()
        cov = e.contig_coverage()
        pos, s0, s1 = e.map_reads(np.array(query, np.int64), (t0, t1))
    c = contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, case["f"])
    tag = case["name"]
    assert (c["P"], c["max_pos"], c["n_freq_kmers"]) == (want["P"], want["max_pos"], want["n_freq_kmers"]), f"{tag}: numpy contig vs reference"
    assert (info["n_positions"], info["max_pos"], info["n_freq_kmers"], info["n_pairs"]) == (want["P"], want["max_pos"], want["n_freq_kmers"], c["n_pairs"]), \
        f"{tag}: device contig {info} vs reference {want['P'], want['max_pos'], want['n_freq_kmers']}"
    want_cov = np.zeros(want["max_pos"] + 1 if want["P"] else 0, np.int32)
    for p, n in want["coverage"]:
        want_cov[p] = n
    assert np.array_equal(c["coverage"], want_cov), f"{tag}: numpy coverage"
    assert np.array_equal(cov, want_cov), f"{tag}: device coverage"
    expect = [tuple(v) if v is not None else (-1, 0, 0) for v in want["reads"].values()]
    assert map_all(unit_ptr, cloud_ptr, entries, c, query, t0, t1) == expect, f"{tag}: numpy answers vs reference"
    got = list(zip(pos.tolist(), s0.tolist(), s1.tolist()))
    bad = [(r_id, g, w) for r_id, g, w in zip(want["reads"], got, expect) if g != w]
    assert not bad, f"{tag} (window {window}): {len(bad)} reads differ from the reference, first {bad[:3]}"
    if log is not None:
        log.append(dict(case=tag, window=window, P=want["P"], mapped=sum(1 for x in expect if x[0] >= 0), reads=len(expect)))
    info["multi_window_reads"] = sum(1 for r in query if hit_span(unit_ptr, cloud_ptr, entries, c, r) > (window or DEFAULT_WINDOW))
    return info

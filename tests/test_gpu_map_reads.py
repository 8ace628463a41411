"""cf_contig_build / cf_map_reads (cf_map.hip) on a real MI355X.

  * every golden case of tests/golden/map_reads_cases.json (the REFERENCE's recorded answers: cloud_contig.py's CloudContig and
    map_reads_fast) with the default window and with windows of 3 and 1 candidate starts;
  * at size: the 50 000 reads of the benchmark and their greedy placement (input data here, not the expectation): the contig of
    all placed reads against the numpy contig of tests/mapcheck.py (figures and the whole coverage), and (pos, s0, s1) of a
    seeded sample of 500 query reads against mapcheck, with the default window and a window of 64.  The share of reads that map
    onto their greedy position is written down (out/map_reads_50k.json, and printed), not asserted: nothing defines what it should be.
Nothing here reads the reference tree."""
import json
import os
import time

import numpy as np
import pytest

import mapcheck
from centroflye_amd import _host, session
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mapcheck.load_cases()
P = dict(k=19, max_nonuniq=3, lo=10, hi=32, min_d=1, max_d=150, min_cov=4, rel_threshold=0.8)


@pytest.fixture(scope="module")
def src(report):
    session.reset()
    session._engine = Engine(0)
    yield mapcheck.Sources(session._engine, report, CASES)
    session.reset()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("window", [0, 3, 1])
def test_every_golden_case_on_the_gpu(src, window):
    assert "gfx950" in src.engine.device_info()["name"]
    several = 0
    for case in CASES["cases"]:
        several += mapcheck.check_case(src, case, window=window)["multi_window_reads"]
    assert len(CASES["cases"]) >= 130
    assert window == 0 or several > len(CASES["cases"])


@pytest.mark.timeout(600)
def test_50k_bench_reads_onto_the_contig_of_their_greedy_placement():
    pk = _host.synth(n_reads=50000, seed=2, n_units=15000, var_len=8)      # the bench workload itself
    e = Engine(0)
    try:
        e.load(pk, 1)
        e.count_kmers(P["k"])
        e.select_rare(P["max_nonuniq"], P["lo"], P["hi"])
        e.build_clouds()
        e.reset_unique()
        e.dist_edges(0, 2 ** 62, P["min_d"], P["max_d"], P["min_cov"], P["rel_threshold"], 0, 1, edge_cap=0)
        gk = e.kmers()[e.unique_mask()]
        e.set_kmers(gk, P["k"])
        e.build_clouds()
        e.filter_clouds(2)
        cp, ent = e.clouds()
        up = np.asarray(pk.units(1)[0], np.int64)
        cls = pk.classify(50000)
        rank = np.argsort(np.argsort(np.array(pk.ids, dtype=object), kind="stable"), kind="stable").astype(np.int32)
        rd, pos, s0, s1 = e.place_reads(cls, rank, 2, 2, 10, 3)
        place_ms = e.times()["place_ms"]
        placed = pos >= 0
        assert placed.sum() > 45000
        b_reads, b_pos = rd[placed], pos[placed]
        e.contig_build(b_reads, b_pos, 2)
        info = e.contig_info()
        cov = e.contig_coverage()
        t = time.time()
        c = mapcheck.contig(up, cp, ent, b_reads, b_pos, 2)
        numpy_s = time.time() - t
        # (the numpy contig of ALL reads is compared whatever it took; numpy_contig_s of the record says how long that was)
        assert (info["n_positions"], info["max_pos"], info["n_freq_kmers"], info["n_pairs"]) == (c["P"], c["max_pos"], c["n_freq_kmers"], c["n_pairs"])
        assert np.array_equal(cov, c["coverage"])
        got = e.map_reads(None, (5, 10))
        map_ms = e.contig_info()["map_ms"]
        sample = np.sort(np.random.default_rng(7).choice(pk.n_reads, 500, replace=False))
        want = mapcheck.map_all(up, cp, ent, c, sample, 5, 10)
        assert [tuple(int(a[r]) for a in got) for r in sample] == want
        assert sum(1 for w in want if w[0] >= 0) > 400
        # the same with a window of 64 starts, queries given as the sample in reverse
        with e.knobs(map_window=64):
            small = e.map_reads(sample[::-1], (5, 10))
        assert [tuple(int(a[i]) for a in small) for i in range(sample.size)] == want[::-1]
        spans = [mapcheck.hit_span(up, cp, ent, c, int(r)) for r in sample]
        greedy = np.full(pk.n_reads, -1, np.int64)
        greedy[rd] = pos
        rec = dict(reads=int(pk.n_reads), placed_by_the_greedy_loop=int(placed.sum()), mapped=int((got[0] >= 0).sum()),
                   mapped_onto_their_greedy_position=int(((got[0] >= 0) & (got[0] == greedy)).sum()),
                   mapped_among_the_greedy_none=int(((got[0] >= 0) & (greedy < 0)).sum()), contig=info,
                   place_device_ms=place_ms, contig_build_ms=info["build_ms"], map_ms=map_ms, numpy_contig_s=round(numpy_s, 2),
                   numpy_contig_reads=int(pk.n_reads), sample=500, sample_hit_span_max=int(max(spans)),
                   sample_reads_spanning_more_than_64_starts=int(sum(1 for x in spans if x > 64)))
        os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
        with open(os.path.join(ROOT, "out", "map_reads_50k.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
    finally:
        e.close()

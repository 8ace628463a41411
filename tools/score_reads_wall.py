#!/usr/bin/env python3
"""Device time of the exact scorer (cf_score_reads) on the benchmark's reads, beside the fast mapper's and the contig build.

One process, one GPU: the bench's reads, stage 2 up to the genomic k-mers, the stage-3 clouds and the greedy placement as in
tools/map_reads_wall.py, then, after `--warmup` rounds, `--reps` rounds (median, minimum, maximum) of
  * cf_contig_build of every placed read (it builds both CSRs): build_ms;
  * cf_map_reads of ALL reads, thresholds (5, 10): map_ms;
  * cf_score_reads of ALL reads over map_reads' range [0, max_pos - units + 1], thresholds (5, 10): score_all_ms;
  * cf_score_reads of the placed reads at their own position, lo = hi = pos, thresholds (0, 0): score_placed_ms;
and what the answers say: how many reads the two mappers place differently (map_reads_fast(debug=True)'s list), what the
reference's map_reads keeps, and how the placed reads score where the greedy loop put them.
No bar: nothing here has been timed before.

    python3 tools/score_reads_wall.py [--reads 50000] [--out profiles/r11_score_reads.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centroflye_amd import _host  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402
from centroflye_amd.read_mapper import kept_by_map_reads  # noqa: E402

P = dict(k=19, max_nonuniq=3, lo=10, hi=32, min_d=1, max_d=150, min_cov=4, rel_threshold=0.8)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_score_reads.json"))
    a = ap.parse_args()
    pk = _host.synth(n_reads=a.reads, seed=a.seed, n_units=max(24, int(round(0.3 * a.reads))), var_len=8)
    with Engine(0) as e:
        dev = e.device_info()
        e.load(pk, 1)
        e.count_kmers(P["k"])
        e.select_rare(P["max_nonuniq"], P["lo"], P["hi"])
        e.build_clouds()
        e.reset_unique()
        e.dist_edges(0, 2 ** 62, P["min_d"], P["max_d"], P["min_cov"], P["rel_threshold"], 0, 1, edge_cap=0)
        gk = e.kmers()[e.unique_mask()]
        e.set_kmers(gk, P["k"])
        e.build_clouds()
        n_entries = e.filter_clouds(2)
        cls = pk.classify(50000)
        rank = np.argsort(np.argsort(np.array(pk.ids, dtype=object), kind="stable"), kind="stable").astype(np.int32)
        rd, pos, s0, s1 = e.place_reads(cls, rank, 2, 2, 10, 3)
        placed = pos >= 0
        b_reads, b_pos = rd[placed], pos[placed]
        t = dict(build_ms=[], map_ms=[], score_all_ms=[], score_placed_ms=[])
        for it in range(a.warmup + a.reps):
            e.contig_build(b_reads, b_pos, 2)
            fast = e.map_reads(None, (5, 10))
            info = e.contig_info()
            exact = e.score_reads(None, None, None, 5, 10)
            all_ms = e.contig_exact_info()["score_ms"]
            own = e.score_reads(b_reads, b_pos, b_pos, 0, 0)
            xinfo = e.contig_exact_info()
            if it >= a.warmup:
                t["build_ms"].append(info["build_ms"])
                t["map_ms"].append(info["map_ms"])
                t["score_all_ms"].append(all_ms)
                t["score_placed_ms"].append(xinfo["score_ms"])
        inner = e.score_reads(None, None, None, 2, 10)
        spread_counts = {str(m): int(e.contig_spread(m).size) for m in (0, 1, 5)}
    mapped = fast[0] >= 0
    differ = mapped & ((fast[0] != exact[0]) | (fast[1] != exact[1]) | (fast[2] != exact[2]))
    keep = kept_by_map_reads(*inner, (5, 10))
    assert (own[0] == b_pos).all()      # thresholds (0, 0) over one start: that start
    rec = dict(device=dev["name"], reads=int(pk.n_reads), bases=int(pk.n_bases), genomic_kmers=int(gk.size), cloud_entries=int(n_entries),
               placed_by_the_greedy_loop=int(placed.sum()), thresholds=[5, 10], min_cloud_kmer_freq=2,
               contig=dict(P=info["n_positions"], max_pos=info["max_pos"], n_freq_kmers=info["n_freq_kmers"], n_pairs=info["n_pairs"],
                           n_exact_pairs=xinfo["n_exact_pairs"], spread_kmers=spread_counts),
               **{k: spread(v) for k, v in t.items()},
               fast=dict(mapped=int(mapped.sum())),
               exact_same_range_and_thresholds=dict(mapped=int((exact[0] >= 0).sum()), fast_mapped_with_another_position=int((mapped & (fast[0] != exact[0])).sum()),
                                                    fast_mapped_with_another_position_or_score=int(differ.sum()),
                                                    mapped_by_one_only=int(((fast[0] >= 0) != (exact[0] >= 0)).sum())),
               map_reads_threshold_5_10=dict(kept=int(keep.sum()), kept_at_another_position_than_fast=int((keep & mapped & (inner[0] != fast[0])).sum()),
                                             kept_but_not_mapped_by_fast=int((keep & ~mapped).sum())),
               placed_reads_at_their_own_position=dict(reads=int(b_reads.size), without_a_hit=int((own[2] == 0).sum()),
                                                       s0_median=float(np.median(own[1])), s1_median=float(np.median(own[2])),
                                                       below_2_10=int(((own[1] < 2) | (own[2] < 10)).sum())),
               method=f"HIP events around each call; {a.warmup} warm-up rounds, then {a.reps} rounds (median, min, max), one process")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

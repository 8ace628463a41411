#!/usr/bin/env python3
"""Device time of the batch mapping (cf_contig_build + cf_map_reads) on the benchmark's reads, beside the greedy loop's.

One process, one GPU: the bench's reads (tests/test_gpu_fullsize.py's synth), stage 2 up to the genomic k-mers, the stage-3
clouds, then
  * the greedy placement (cf_place_reads): place_device_ms, `--reps` times;
  * the contig of every placed read and the mapping of ALL reads, thresholds (5, 10): build_ms and map_ms, after `--warmup` calls,
    `--reps` times each (median, minimum, maximum);
  * the size of the work, counted on the host from the CSR: records sorted, seed pairs, hits accumulated, windows per read,
    and the algorithmic bytes of both kernels' streams with their fraction of 8 TB/s.
The one bar: build_ms + map_ms (medians) below place_device_ms (median) — a batch map has no R-step dependent chain.

    python3 tools/map_reads_wall.py [--reads 50000] [--out profiles/r10_map_reads.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapcheck  # noqa: E402
from centroflye_amd import _host  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

P = dict(k=19, max_nonuniq=3, lo=10, hi=32, min_d=1, max_d=150, min_cov=4, rel_threshold=0.8)
HBM_BYTES_PER_S = 8e12
WINDOW = 2048


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))


def work(up, cp, ent, c, n_reads, chunk=2000):
    """Hits (seed, unit) pairs with q >= i and s + n <= P, and passes over windows, over all reads."""
    hits = visits = windows = mapped_span = 0
    for lo in range(0, n_reads, chunk):
        hi = min(n_reads, lo + chunk)
        units, u_read = mapcheck._ranges(up[lo:hi], up[lo + 1:hi + 1])
        ents, e_unit = mapcheck._ranges(cp[units], cp[units + 1])
        x = ent[ents]
        seeds, owner = mapcheck._ranges(np.searchsorted(c["seed_rank"], x, "left"), np.searchsorted(c["seed_rank"], x, "right"))
        read = u_read[e_unit[owner]]
        i = units[e_unit[owner]] - up[lo:hi][read]
        s = c["seed_pos"][seeds] - i
        n = (up[lo + 1:hi + 1] - up[lo:hi])[read]
        ok = (s >= 0) & (s + n <= c["P"])
        visits += int(seeds.size)
        hits += int(ok.sum())
        smin = np.full(hi - lo, np.iinfo(np.int64).max)
        smax = np.full(hi - lo, -1)
        np.minimum.at(smin, read[ok], s[ok])
        np.maximum.at(smax, read[ok], s[ok])
        has = smax >= 0
        windows += int(((smax[has] - smin[has]) // WINDOW + 1).sum())
        mapped_span += int(has.sum())
    return dict(seed_visits_per_pass=visits, hits_accumulated=hits, reads_with_a_hit=mapped_span, windows=windows,
                windows_per_read_with_a_hit=round(windows / max(1, mapped_span), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--place-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_map_reads.json"))
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
        cp, ent = e.clouds()
        up = np.asarray(pk.units(1)[0], np.int64)
        cls = pk.classify(50000)
        rank = np.argsort(np.argsort(np.array(pk.ids, dtype=object), kind="stable"), kind="stable").astype(np.int32)
        place = []
        for _ in range(a.place_reps):
            rd, pos, s0, s1 = e.place_reads(cls, rank, 2, 2, 10, 3)
            place.append(e.times()["place_ms"])
        placed = pos >= 0
        b_reads, b_pos = rd[placed], pos[placed]
        build, mapt = [], []
        for it in range(a.warmup + a.reps):
            e.contig_build(b_reads, b_pos, 2)
            got = e.map_reads(None, (5, 10))
            info = e.contig_info()
            if it >= a.warmup:
                build.append(info["build_ms"])
                mapt.append(info["map_ms"])
    c = mapcheck.contig(up, cp, ent, b_reads, b_pos, 2)
    assert (info["n_positions"], info["max_pos"], info["n_freq_kmers"], info["n_pairs"]) == (c["P"], c["max_pos"], c["n_freq_kmers"], c["n_pairs"])
    w = work(up, cp, ent.astype(np.int64), c, pk.n_reads)
    n_rec = int((cp[up[b_reads + 1]] - cp[up[b_reads]]).sum())
    K = int(gk.size)
    bits = max(1, int(c["max_pos"]).bit_length()) + max(1, int(max(K - 1, 0)).bit_length())
    passes = (bits + 7) // 8
    # build: the emit pass (entry 4 B in, record 8 B out), per radix pass one read for the histogram and a read + a write for the
    # scatter (24 B a record), the three passes over the sorted records (8 B each, + 4 B flag out / in, 8 B offset out / in) and
    # the CSR (8 B per rank, 4 B per pair)
    build_bytes = n_rec * (12 + 24 * passes + 3 * 8 + 2 * 4 + 2 * 8) + 8 * (K + 1) + 4 * c["n_pairs"]
    # map: per pass over a read (the span pass + one per window) its entries (4 B) and their two row offsets (16 B), 4 B per seed
    # looked at; 20 B of results per read
    entry_visits = int(n_entries) * (1 + w["windows"] / max(1, w["reads_with_a_hit"]))
    map_bytes = int(entry_visits * 20 + w["seed_visits_per_pass"] * 4 * (1 + w["windows"] / max(1, w["reads_with_a_hit"])) + 20 * pk.n_reads)
    b, m, g = statistics.median(build), statistics.median(mapt), statistics.median(place)
    greedy = np.full(pk.n_reads, -1, np.int64)
    greedy[rd] = pos
    rec = dict(device=dev["name"], reads=int(pk.n_reads), bases=int(pk.n_bases), genomic_kmers=K, cloud_entries=int(n_entries),
               placed_by_the_greedy_loop=int(placed.sum()), thresholds=[5, 10], min_cloud_kmer_freq=2, map_window=WINDOW,
               place_device_ms=spread(place), build_ms=spread(build), map_ms=spread(mapt),
               build_plus_map_ms=round(b + m, 3), below_place_device_ms=bool(b + m < g), place_over_build_plus_map=round(g / (b + m), 1),
               records_sorted=n_rec, sort_key_bits=bits, radix_passes=passes, contig=dict(P=c["P"], max_pos=c["max_pos"],
               n_freq_kmers=c["n_freq_kmers"], n_pairs=c["n_pairs"]), work=w,
               algorithmic_bytes=dict(build=int(build_bytes), map=int(map_bytes),
                                      build_fraction_of_8TBps=round(build_bytes / (b * 1e-3) / HBM_BYTES_PER_S, 4),
                                      map_fraction_of_8TBps=round(map_bytes / (m * 1e-3) / HBM_BYTES_PER_S, 4)),
               mapped=int((got[0] >= 0).sum()), mapped_onto_their_greedy_position=int(((got[0] >= 0) & (got[0] == greedy)).sum()),
               mapped_among_the_greedy_none=int(((got[0] >= 0) & (greedy < 0)).sum()),
               method=f"HIP events around each call; {a.warmup} warm-up calls, then {a.reps} repetitions (median, min, max); the greedy loop {a.place_reps} times in the same process")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Goldens of the batch mapping onto a finished cloud contig, captured from the REFERENCE ITSELF (build container only: imports
the reference's scripts read-only through make_golden.import_reference).

For every case the reference's own objects are driven: CloudContig(f), add_read(read, pos) for every backbone read
(cloud_contig.py:26-41), then map_reads_fast(contig, reads, threshold) (:117-156).  Recorded: P = len(contig.clouds), max_pos,
len(freq_kmers), the coverage, and (pos, s0, s1) — or null — of every query read.

Sources of clouds:
  * the fixtures tiny, hor2055, lowcov with the reference's unique k-mers (tests/golden/<name>.unique_kmers.txt), clouds after the
    multiplicity filter, as read_placer.py:103-108 builds them; tiny again with --n-motif 2; exotic_rare (k-mers with an N);
  * `hand`: a hand-built array of 40 positions — one k-mer of its own per position, five k-mers that recur with period 5, and the
    positions 20 .. 24 repeating the own k-mers of 5 .. 9 — read by windows, plus a read without units and one whose clouds are
    all empty.
Cases:
  * per fixture the full contig (backbone = the placed lines of the fixture's golden read_positions), f = 2, thresholds (5, 10)
    and (2, 10);
  * per fixture N_RANDOM seeded cases: a random quarter / half / three quarters / all of the placed reads as the backbone,
    f in {1, 2, 3}, thresholds in {(5, 10), (2, 10), (1, 1), (3, 30)};
  * hand-built backbones: two with a coverage gap (P < max_pos + 1) where `s + n <= P` decides a read, a tie between two starts,
    a k-mer that is frequent at one place and present once at another, a unit with an empty cloud that covers a position, an
    empty backbone.
tests/mapcheck.py can plant five misreadings of the reference; `wrong_rule_kills` records in how many cases of each source the
answers of some read change.  Every misreading must change at least one case, or this script fails.

    PYTHONHASHSEED=1 python tests/golden/make_golden_map_reads.py
    PYTHONHASHSEED=2 python tests/golden/make_golden_map_reads.py --check      # must print IDENTICAL
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import fixtures  # noqa: E402
import mapcheck  # noqa: E402
from make_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "map_reads_cases.json")
N_RANDOM = 40
THRESHOLDS = [(5, 10), (2, 10), (1, 1), (3, 30)]
FIXTURE_SOURCES = {      # name -> (fixture, n_motif, golden with the placed lines)
    "tiny": ("tiny", 1, "tiny.json"),
    "hor2055": ("hor2055", 1, "hor2055.json"),
    "lowcov": ("lowcov", 1, "lowcov.json"),
    "tiny_n_motif2": ("tiny", 2, "tiny.n_motif2.json"),
    "exotic_rare": ("exotic_rare", 1, "exotic_rare.json"),
}


def placed_lines(golden_file):
    with open(os.path.join(HERE, golden_file)) as f:
        g = json.load(f)
    out = []
    for ln in g["read_positions"]["placed"]:
        fields = ln.split(" ")
        out.append([fields[0], int(fields[1])])
    return out


def reference_clouds(name, workdir):
    """{r_id: ReadKMerCloud} of the reference for a fixture source, in report order, and the CSR of the same clouds."""
    ncrf_parser, D, RP, RKC, CC = import_reference()
    fixture, n_motif, _ = FIXTURE_SOURCES[name]
    p3 = fixtures.stage3_params(fixture)
    with open(os.path.join(HERE, f"{fixture}.unique_kmers.txt")) as f:
        gk = set(ln.strip() for ln in f if ln.strip())
    rep = ncrf_parser.NCRF_Report(fixtures.make_report(fixture, workdir))
    with contextlib.redirect_stdout(io.StringIO()):
        clouds = RKC.get_reads_kmer_clouds(rep, n=n_motif, k=p3["k_cloud"], genomic_kmers=gk)
        clouds = RKC.filter_reads_kmer_clouds(clouds, min_mult=p3["min_kmer_mult"])
    ordered = {r_id: clouds[r_id] for r_id in rep.records}
    spec = dict(kind="fixture", fixture=fixture, kmers_file=f"{fixture}.unique_kmers.txt", n_motif=n_motif, k_cloud=p3["k_cloud"],
                min_kmer_mult=p3["min_kmer_mult"])
    return ordered, spec


def hand_source():
    """The hand-built array (see the module docstring): content[p] = ranks at array position p; reads are windows of it."""
    content = [[p, 40 + p % 5] for p in range(40)]
    for j in range(5):
        content[20 + j][0] = 5 + j
    windows = [(0, 8), (0, 8), (4, 8), (4, 8), (12, 8), (12, 8), (18, 8), (18, 8), (5, 5), (14, 5), (12, 3), (0, 5), None, "empty3",
               (26, 6), (2, 4), (30, 8), (30, 8)]
    unit_ptr, cloud_ptr, entries = [0], [0], []
    for w in windows:
        units = [] if w is None else ([[], [], []] if w == "empty3" else [sorted(content[p]) for p in range(w[0], w[0] + w[1])])
        for u in units:
            entries.extend(u)
            cloud_ptr.append(len(entries))
        unit_ptr.append(len(cloud_ptr) - 1)
    spec = dict(kind="synthetic", unit_ptr=unit_ptr, cloud_ptr=cloud_ptr, entries=entries, K=45)
    clouds = {}
    for r in range(len(windows)):
        kmers = [set(f"x{e:02d}" for e in entries[cloud_ptr[u]:cloud_ptr[u + 1]]) for u in range(unit_ptr[r], unit_ptr[r + 1])]
        clouds[str(r)] = types.SimpleNamespace(r_id=str(r), kmers=kmers)
    return clouds, spec


HAND_CASES = [      # name, backbone [(read, pos)], f, threshold
    # array 12 .. 19 laid on 14 .. 21: positions 8 .. 13 are not covered, P = 16 < max_pos + 1 = 22; read 9 (array 14 .. 18) has its
    # hits at start 16, and 16 + 5 > 16
    ("hand_gap_a", [("0", 0), ("1", 0), ("4", 14), ("5", 14)], 2, (2, 2)),
    # array 30 .. 37 laid far out; read 13 (three empty clouds) covers 8 .. 10 although it holds no k-mer
    ("hand_gap_b", [("0", 0), ("1", 0), ("16", 50), ("17", 50), ("13", 8)], 1, (1, 1)),
    # every window at its own place: read 8 (own k-mers of 5 .. 9 = those of 20 .. 24) ties between the starts 5 and 20
    ("hand_tie", [("0", 0), ("1", 0), ("2", 4), ("3", 4), ("4", 12), ("5", 12), ("6", 18), ("7", 18)], 2, (2, 2)),
    # the recurring k-mers are frequent on 0 .. 7 and present ONCE on 12 .. 19: read 9 maps through the latter
    ("hand_frequent_elsewhere", [("0", 0), ("1", 0), ("4", 12)], 2, (2, 2)),
    ("hand_frequent_elsewhere_f3", [("0", 0), ("1", 0), ("11", 0), ("4", 12), ("6", 18)], 3, (1, 1)),
    ("hand_empty_backbone", [], 2, (1, 1)),
    ("hand_only_empty_clouds", [("13", 3), ("12", 0)], 1, (1, 1)),
]


def run_reference(CC, clouds, backbone, f, threshold):
    cc = CC.CloudContig(f)
    for r_id, pos in backbone:
        cc.add_read(clouds[r_id], pos)
    with contextlib.redirect_stdout(io.StringIO()):
        positions, scores = CC.map_reads_fast(cc, clouds, threshold=tuple(threshold))
    reads = {}
    for r_id, c in clouds.items():
        if r_id in positions:
            by_unit = scores[r_id][positions[r_id]]
            reads[r_id] = [positions[r_id], len(by_unit), sum(by_unit.values())]
        else:
            reads[r_id] = None
    return dict(P=len(cc.clouds), max_pos=cc.max_pos, n_freq_kmers=len(cc.freq_kmers),
                coverage=sorted([p, n] for p, n in cc.coverage.items()), reads=reads)


def csr_of(clouds):
    """CSR with ranks of the sorted k-mer strings (only the grouping of equal k-mers matters to the mapping)."""
    names = sorted(set(k for c in clouds.values() for u in c.kmers for k in u))
    rank = {k: i for i, k in enumerate(names)}
    unit_ptr, cloud_ptr, entries = [0], [0], []
    for c in clouds.values():
        for u in c.kmers:
            entries.extend(sorted(rank[k] for k in u))
            cloud_ptr.append(len(entries))
        unit_ptr.append(len(cloud_ptr) - 1)
    return np.array(unit_ptr, np.int64), np.array(cloud_ptr, np.int64), np.array(entries, np.int64)


def capture():
    CC = import_reference()[4]
    sources, cases, kills = {}, [], {w: {} for w in mapcheck.WRONG_RULES}
    with tempfile.TemporaryDirectory() as wd:
        plan = []
        for name, (fixture, n_motif, gfile) in FIXTURE_SOURCES.items():
            clouds, spec = reference_clouds(name, wd)
            sources[name] = spec
            placed = placed_lines(gfile)
            todo = [(f"{name}_full_t5_10", placed, 2, (5, 10)), (f"{name}_full_t2_10", placed, 2, (2, 10))]
            if name in fixtures.FIXTURES:
                rng = random.Random(f"map_reads {name}")
                for j in range(N_RANDOM):
                    frac = rng.choice([0.25, 0.5, 0.75, 1.0])
                    sub = sorted(rng.sample(range(len(placed)), max(1, round(frac * len(placed)))))
                    todo.append((f"{name}_random{j:02d}", [placed[i] for i in sub], rng.choice([1, 2, 3]), rng.choice(THRESHOLDS)))
            plan.append((name, clouds, todo))
        clouds, spec = hand_source()
        sources["hand"] = spec
        plan.append(("hand", clouds, HAND_CASES))
        for name, clouds, todo in plan:
            unit_ptr, cloud_ptr, entries = csr_of(clouds)
            ids = list(clouds)
            row = {r_id: i for i, r_id in enumerate(ids)}
            for w in mapcheck.WRONG_RULES:
                kills[w][name] = 0
            for cname, backbone, f, thr in todo:
                backbone = [[r, int(p)] for r, p in backbone]
                want = run_reference(CC, clouds, backbone, f, thr)
                cases.append(dict(name=cname, source=name, backbone=backbone, f=f, threshold=list(thr), expect=want))
                expect = [tuple(v) if v is not None else (-1, 0, 0) for v in want["reads"].values()]
                b_reads, b_pos = [row[r] for r, _ in backbone], [p for _, p in backbone]
                for w in (None,) + mapcheck.WRONG_RULES:
                    c = mapcheck.contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, f, wrong=w)
                    got = mapcheck.map_all(unit_ptr, cloud_ptr, entries, c, range(len(ids)), thr[0], thr[1], wrong=w)
                    if w is None:
                        assert got == expect and (c["P"], c["max_pos"], c["n_freq_kmers"]) == (want["P"], want["max_pos"], want["n_freq_kmers"]), \
                            f"{cname}: the numpy statement differs from the reference"
                    elif got != expect:
                        kills[w][name] += 1
    for w, per in kills.items():
        assert sum(per.values()) > 0, f"no case tells the wrong rule '{w}' from the reference: add one"
    gaps = [c["name"] for c in cases if c["expect"]["P"] and c["expect"]["P"] < c["expect"]["max_pos"] + 1]
    return dict(sources=sources, cases=cases, wrong_rule_kills=kills, cases_with_a_coverage_gap=gaps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed file")
    a = ap.parse_args()
    g = capture()
    text = json.dumps(g, sort_keys=True, separators=(",", ":"))
    if a.check:
        with open(OUT) as f:
            same = json.dumps(json.load(f), sort_keys=True, separators=(",", ":")) == text
        print(f"map_reads_cases: {'IDENTICAL' if same else 'DIFFERENT'} under PYTHONHASHSEED={os.environ.get('PYTHONHASHSEED', '')}")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"wrote {OUT}: {len(g['cases'])} cases, {os.path.getsize(OUT)} bytes; gap cases {g['cases_with_a_coverage_gap']}")
    for w, per in g["wrong_rule_kills"].items():
        print(f"  {w}: {per}")


if __name__ == "__main__":
    main()

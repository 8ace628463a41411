#!/usr/bin/env python3
"""Goldens of the EXACT scorer of a finished cloud contig, captured from the REFERENCE ITSELF (build container only: imports the
reference's scripts read-only through make_golden.import_reference).

The sources of clouds and the backbones are those of make_golden_map_reads.py: a case here names the case of
map_reads_cases.json it is built on (`of`: its source, backbone and f) and carries thresholds of its own.  For every case the
reference's own objects are driven: CloudContig(f), add_read(read, pos) for every backbone read (cloud_contig.py:26-41), then per
read, as one flat row of integers (a position None is -1):
  [0:3]    calc_inters_score over [0, max_pos - n + 1], the case's thresholds (:46-76; map_reads' range, what debug compares with);
  [3:6]    the same over [0, max_pos]: the read overhangs the contig and is truncated (:57);
  [6:11]   a, b and the answer over the seeded sub-range [a, b] (b may lie beyond max_pos);
  [11:15]  c and the answer over the single start [c, c] under the thresholds (0, 0): the score of the read AT c;
  [15:]    map_reads(threshold = the case's) (:98-114): 1, pos, s0, s1 when the read is kept, 0 when it is not.
Per case also max_pos, n_exact_pairs = sum of len(freq_clouds[p]), and for get_spread_kmers(max_npos), max_npos in {0, 1, 5}
(:78-84): how many k-mers, how many positions they have in all, and how many cloud entries of all reads hold one (the k-mers'
names are strings of the reference; the figures do not depend on how they are ranked).
Cases: per fixture the full contig under its two map thresholds (so that the recorded fast answers can be compared), N_RANDOM of
the random backbones of the map goldens under seeded thresholds that include (0, 0), the seven hand-built backbones, and
`hand_tie` again under (8, 16) and (5, 10), where reads score exactly the threshold.
tests/scorecheck.py can plant seven misreadings of the reference; `wrong_rule_kills` records in how many cases of each source
some row changes.  Every misreading must change at least one case, or this script fails.

    PYTHONHASHSEED=1 python tests/golden/make_golden_score_reads.py
    PYTHONHASHSEED=2 python tests/golden/make_golden_score_reads.py --check      # must print IDENTICAL
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import fixtures  # noqa: E402
import make_golden_map_reads as mg  # noqa: E402
import scorecheck  # noqa: E402
from make_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "score_reads_cases.json")
N_RANDOM = 12
THRESHOLDS = [(5, 10), (2, 10), (1, 1), (0, 0), (3, 30)]
HAND_AGAIN = [("hand_tie", (8, 16)), ("hand_tie", (5, 10)), ("hand_gap_a", (0, 0)), ("hand_only_empty_clouds", (0, 0))]


def triple(answer):
    score, pos = answer
    return [-1 if pos is None else int(pos), int(score[0]), int(score[1])]


def run_reference(CC, clouds, order, backbone, f, threshold, rng):
    cc = CC.CloudContig(f)
    for r_id, pos in backbone:
        cc.add_read(clouds[r_id], pos)
    t0, t1 = threshold
    with contextlib.redirect_stdout(io.StringIO()):
        kept_pos, kept_score = CC.map_reads(cc, clouds, threshold=tuple(threshold))
    rows = []
    for r_id in order:      # (the read order of the map golden: its keys, sorted)
        c = clouds[r_id]
        n = len(c.kmers)
        a = rng.randint(0, cc.max_pos)
        b = rng.randint(a, cc.max_pos + 3)
        c0 = rng.randint(0, cc.max_pos + 1)
        row = triple(cc.calc_inters_score(c, max_position=cc.max_pos - n + 1, min_unit=t0, min_inters=t1))
        row += triple(cc.calc_inters_score(c, max_position=cc.max_pos, min_unit=t0, min_inters=t1))
        row += [a, b] + triple(cc.calc_inters_score(c, min_position=a, max_position=b, min_unit=t0, min_inters=t1))
        row += [c0] + triple(cc.calc_inters_score(c, min_position=c0, max_position=c0, min_unit=0, min_inters=0))
        row += [1] + triple((kept_score[r_id], kept_pos[r_id])) if r_id in kept_pos else [0]
        rows.append(row)
    spread = {}
    for m in scorecheck.SPREAD_MAX_NPOS:
        ks = cc.get_spread_kmers(m)
        spread[str(m)] = [len(ks), sum(len(cc.kmer_positions[k]) for k in ks), sum(1 for c in clouds.values() for u in c.kmers for k in u if k in ks)]
    return dict(max_pos=cc.max_pos, n_exact_pairs=sum(len(v) for v in cc.freq_clouds.values()), spread=spread, reads=rows)


def capture():
    CC = import_reference()[4]
    with open(mg.OUT) as f:
        base = {c["name"]: c for c in json.load(f)["cases"]}
    cases, kills = [], {w: {} for w in scorecheck.WRONG_RULES}
    with tempfile.TemporaryDirectory() as wd:
        plan = []
        for name in mg.FIXTURE_SOURCES:
            clouds, _ = mg.reference_clouds(name, wd)
            todo = [(f"{name}_full_t5_10", f"{name}_full_t5_10", (5, 10)), (f"{name}_full_t2_10", f"{name}_full_t2_10", (2, 10))]
            if name in fixtures.FIXTURES:
                rng = random.Random(f"score_reads {name}")
                for j in sorted(rng.sample(range(mg.N_RANDOM), N_RANDOM)):
                    todo.append((f"{name}_random{j:02d}", f"{name}_random{j:02d}", rng.choice(THRESHOLDS)))
            plan.append((name, clouds, todo))
        clouds, _ = mg.hand_source()
        todo = [(c[0], c[0], c[3]) for c in mg.HAND_CASES] + [(f"{n}_t{t[0]}_{t[1]}", n, t) for n, t in HAND_AGAIN]
        plan.append(("hand", clouds, todo))
        for name, clouds, todo in plan:
            unit_ptr, cloud_ptr, entries = mg.csr_of(clouds)
            ids = list(clouds)
            row = {r_id: i for i, r_id in enumerate(ids)}
            for w in scorecheck.WRONG_RULES:
                kills[w][name] = 0
            for cname, of, thr in todo:
                b = base[of]
                order = list(b["expect"]["reads"])
                assert b["source"] == name and sorted(order) == sorted(ids)
                want = run_reference(CC, clouds, order, b["backbone"], b["f"], thr, random.Random(f"score_reads ranges {cname}"))
                cases.append(dict(name=cname, of=of, threshold=list(thr), **want))
                b_reads, b_pos = [row[r] for r, _ in b["backbone"]], [p for _, p in b["backbone"]]
                c = scorecheck.contig(unit_ptr, cloud_ptr, entries, b_reads, b_pos, b["f"])
                assert (c["max_pos"], c["n_exact_pairs"]) == (want["max_pos"], want["n_exact_pairs"]), f"{cname}: numpy contig"
                for m in scorecheck.SPREAD_MAX_NPOS:
                    assert scorecheck.spread_figures(entries, c, m) == want["spread"][str(m)], f"{cname}: numpy spread k-mers {m}"
                for w in (None,) + scorecheck.WRONG_RULES:
                    got = [scorecheck.read_row(unit_ptr, cloud_ptr, entries, c, row[r_id], thr, x[6:8] + [x[11]], wrong=w)
                           for r_id, x in zip(order, want["reads"])]
                    if w is None:
                        bad = [(r_id, g, x) for r_id, g, x in zip(order, got, want["reads"]) if g != x]
                        assert not bad, f"{cname}: the numpy statement differs from the reference: {bad[:3]}"
                    elif got != want["reads"]:
                        kills[w][name] += 1
    for w, per in kills.items():
        assert sum(per.values()) > 0, f"no case tells the wrong rule '{w}' from the reference: add one"
    return dict(cases=cases, wrong_rule_kills=kills)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed file")
    a = ap.parse_args()
    g = capture()
    text = json.dumps(g, sort_keys=True, separators=(",", ":"))
    if a.check:
        with open(OUT) as f:
            same = json.dumps(json.load(f), sort_keys=True, separators=(",", ":")) == text
        print(f"score_reads_cases: {'IDENTICAL' if same else 'DIFFERENT'} under PYTHONHASHSEED={os.environ.get('PYTHONHASHSEED', '')}")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"wrote {OUT}: {len(g['cases'])} cases, {os.path.getsize(OUT)} bytes")
    for w, per in g["wrong_rule_kills"].items():
        print(f"  {w}: {per}")


if __name__ == "__main__":
    main()

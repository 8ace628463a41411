#!/usr/bin/env python3
"""Device time of the built-in consensus polisher (cf_consensus_run) at the cenX shape, the wall time of the stage
around it, and what there is to compare it with.

  (a) 1 500 positions x 32 reads of 2 055-base units at the generator's error rates (2 % deletions, 2 % substitutions, 1.5 %
      insertions; the template of a position is one more such read), 4 iterations: device ms per phase by HIP events
      (cf_consensus_info), median of --reps runs after --warmup;
  (b) the wall time of the stage from the exported tree on: the pos_P/read_units.fasta and median_read_unit.fasta of (a) written
      first, then ELTR_Polisher.run_consensus (FASTA in, one device call, polished_i.fasta and consensus_report.tsv out) and
      assemble (final sequences, report.txt, position_changes.csv) timed;
  (c) Flye is not available, so the only comparison is the rule's plain-Python restatement (tests/conscheck.py) on one host core
      over the first --sample positions, SCALED by full-matrix cells to all of them and labelled as scaled; the device's bytes of
      those positions are checked against it on the way;
  (d) with --bench-tree: the headline of bench.py in this tree and in another BUILT tree (a checkout of the parent commit; its own
      bench.py and library: this tree's binding cannot load a library without the new entry points), alternated, --bench-runs each
      (the headline leg alone: no CPU baseline, no placement, no other workload).

    python tools/consensus_wall.py --out profiles/r15_consensus.json [--bench-tree DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from centroflye_amd import eltr_polisher, session  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def noisy(rng, s, p_del=0.02, p_sub=0.02, p_ins=0.015):
    """A read of the unit s (codes 0 .. 3): substitutions, deletions, inserted bases, whole arrays at a time."""
    s = s.copy()
    sub = rng.random(s.size) < p_sub
    s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    s = s[rng.random(s.size) >= p_del]
    at = np.flatnonzero(rng.random(s.size + 1) < p_ins)
    return np.insert(s, at, rng.integers(0, 4, at.size))


def workload(rng, n_pos, n_reads, unit_len):
    base = rng.integers(0, 4, unit_len)
    templates, reads, truths = [], [], []
    for _ in range(n_pos):
        unit = base.copy()
        p = rng.integers(0, unit_len, unit_len // 50)      # 2 % divergence between the units of the array
        unit[p] = rng.integers(0, 4, p.size)
        truths.append(ACGT[unit].tobytes())
        templates.append(ACGT[noisy(rng, unit)].tobytes())
        reads.append([ACGT[noisy(rng, unit)].tobytes() for _ in range(n_reads)])
    return templates, reads, truths


def pack(templates, reads):
    t_off = np.zeros(len(templates) + 1, np.int64)
    np.cumsum([len(t) for t in templates], out=t_off[1:])
    flat = [r for rs in reads for r in rs]
    r_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(r) for r in flat], out=r_off[1:])
    pos_ptr = np.zeros(len(templates) + 1, np.int64)
    np.cumsum([len(rs) for rs in reads], out=pos_ptr[1:])
    return b"".join(templates), t_off, b"".join(flat), r_off, pos_ptr


def bench_line(tree, steps, warmup):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-place",
           "--steps-b", "0", "--steps-c", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=tree)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed: {p.stderr[-1000:]}")
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return dict(value=line["value"], unit=line.get("unit"), ms_per_step=line.get("ms_per_step"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_consensus.json"))
    ap.add_argument("--positions", type=int, default=1500)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--unit-len", type=int, default=2055)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2, help="positions the restatement is run on (one host core)")
    ap.add_argument("--bench-tree", default=None, help="another built tree (a checkout of the parent commit) to alternate bench.py with")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    args = ap.parse_args()
    rng = np.random.default_rng(15)
    t = time.perf_counter()
    templates, reads, truths = workload(rng, args.positions, args.reads, args.unit_len)
    out = dict(tool="tools/consensus_wall.py", positions=args.positions, reads_per_position=args.reads, unit_len=args.unit_len, iters=args.iters,
               reps=args.reps, warmup=args.warmup, error_rates=dict(deletion=0.02, substitution=0.02, insertion=0.015),
               generate_s=round(time.perf_counter() - t, 2))
    packed = pack(templates, reads)
    with Engine(0) as e:
        out["device"] = e.device_info()
        phases, walls = [], []
        for i in range(args.warmup + args.reps):
            t = time.perf_counter()
            res = e.consensus_run(*packed, n_iters=args.iters, permille=300)
            wall = (time.perf_counter() - t) * 1e3
            if i >= args.warmup:
                phases.append(e.consensus_info()["phase_ms"])
                walls.append(wall)
        info = e.consensus_info()
        out["kernel"] = {k: v for k, v in info.items() if k != "phase_ms"}
        out["a_device_ms_median"] = {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}
        out["a_device_ms_all_total"] = [round(p["total"], 2) for p in phases]
        out["a_call_wall_ms_median"] = round(statistics.median(walls), 2)
        cells = [sum(len(templates[p]) * len(r) for r in reads[p]) for p in range(args.positions)]
        out["a_full_matrix_cells_per_iteration"] = int(sum(cells))
        # quality: positions whose output is the true unit, per iteration; reads that voted
        out["a_positions_equal_to_truth"] = [int(sum(b[off[p]:off[p + 1]].tobytes() == truths[p] for p in range(args.positions))) for b, off, _, _ in res]
        out["a_excluded_reads"] = [int(ne.sum()) for _, _, _, ne in res]
        print("a", json.dumps({k: out[k] for k in out if k.startswith("a_")}), flush=True)

        # (c) the restatement on one core over a sample, scaled by cells
        import conscheck as cc
        t = time.perf_counter()
        sample = list(range(min(args.sample, args.positions)))
        want = [cc.consensus(templates[p], reads[p], args.iters, 300) for p in sample]
        sec = time.perf_counter() - t
        for p, w in zip(sample, want):
            for i, (b, off, nv, ne) in enumerate(res):
                assert (b[off[p]:off[p + 1]].tobytes(), int(nv[p]), int(ne[p])) == w[i], (p, i)
        share = sum(cells[p] for p in sample) / sum(cells)
        out["c_restatement_one_core"] = dict(sample_positions=len(sample), seconds=round(sec, 2), share_of_cells=share,
                                             scaled_to_all_positions_s=round(sec / share, 1), scaled=True,
                                             note="plain Python + numpy full matrices; a statement of the rule, not an optimised CPU polisher",
                                             device_equals_restatement_on_sample=True)
        print("c", json.dumps(out["c_restatement_one_core"]), flush=True)

        # (b) the stage from the exported tree on
        wd = tempfile.mkdtemp(prefix="consensus_wall_")
        try:
            t = time.perf_counter()
            files = {}
            for p in range(args.positions):
                d = os.path.join(wd, f"pos_{p}")
                os.mkdir(d)
                files[p] = (os.path.join(d, "read_units.fasta"), os.path.join(d, "median_read_unit.fasta"))
                with open(files[p][0], "w") as f:
                    f.write("".join(f">read_{q}\n{r.decode()}\n" for q, r in enumerate(reads[p])))
                with open(files[p][1], "w") as f:
                    f.write(f">median\n{templates[p].decode()}\n")
            write_s = time.perf_counter() - t
            pol = object.__new__(eltr_polisher.ELTR_Polisher)
            pol.params = types.SimpleNamespace(outdir=wd, num_iters=args.iters, position_report=True)
            session.reset()
            session._engine = e
            t = time.perf_counter()
            pol.run_consensus(files)
            t1 = time.perf_counter()
            pol.assemble(files)
            t2 = time.perf_counter()
            session._engine = None
            out["b_stage_wall_s"] = dict(tree_written_by_this_tool_s=round(write_s, 2), run_consensus_s=round(t1 - t, 2), assemble_s=round(t2 - t1, 2),
                                         total_s=round(t2 - t, 2), device_ms_inside=pol.consensus_ms,
                                         covers="FASTA of every position read, one cf_consensus_run, polished_i.fasta and consensus_report.tsv written, "
                                                "assemble with --position-report; not the export of the read units from the NCRF report")
            print("b", json.dumps(out["b_stage_wall_s"]), flush=True)
        finally:
            shutil.rmtree(wd, ignore_errors=True)
    if args.bench_tree:
        runs = []
        for i in range(args.bench_runs):
            for name, tree in (("other", os.path.abspath(args.bench_tree)), ("this", ROOT)):
                runs.append(dict(build=name, **bench_line(tree, args.bench_steps, args.bench_warmup)))
                print("d", json.dumps(runs[-1]), flush=True)
        out["d_bench_headline_alternated"] = dict(other_tree=os.path.basename(os.path.abspath(args.bench_tree)), steps=args.bench_steps, warmup=args.bench_warmup, runs=runs,
                                                  median_this=statistics.median(r["value"] for r in runs if r["build"] == "this"),
                                                  median_other=statistics.median(r["value"] for r in runs if r["build"] == "other"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

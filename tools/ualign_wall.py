#!/usr/bin/env python3
"""Device time of the built-in tandem aligner (cf_ualign_run) on the benchmark's own reads, and what there is to
compare it with.

  (a) the reads of bench.py (`_host.synth` with its synth_kwargs; the pack's de-gapped bases as reads, every second one
      reverse-complemented) against the 2 055-base unit: --reads of them (50 000 is the benchmark; 500 is the short run): device ms
      per phase by HIP events (cf_ualign_info), cells per second (2 strands x read bytes x unit bases per score pass; the rows of the
      moves pass on top), reads with a hit, the share of each read's bases inside its interval;
  (b) NCRF is not available, so the only comparison is the rule's numpy restatement (tests/ualigncheck.py) on one host core over
      the first --sample reads, SCALED by cells to all of them and labelled as scaled; the device's hits and ops of those reads
      are checked against it on the way.

    python tools/ualign_wall.py --reads 500 --reads 50000 --out profiles/r22_ualign.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from centroflye_amd import _host  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

_COMP = np.zeros(256, np.uint8)
_COMP[list(b"ACGTacgtNn")] = list(b"TGCAtgcaNn")


def reads_of(n_reads, seed):
    pk = _host.synth(n_reads=n_reads, **bench.synth_kwargs(n_reads, seed))
    bases, off = np.array(pk.bases, np.uint8), np.array(pk.read_off, np.int64)
    for q in range(1, pk.n_reads, 2):
        bases[off[q]:off[q + 1]] = _COMP[bases[off[q]:off[q + 1]]][::-1]
    return pk.motifs[0].encode(), bases, off


def measure(e, n_reads, seed, reps, warmup, sample):
    import ualigncheck as uc
    unit, bases, off = reads_of(n_reads, seed)
    runs = []
    for rep in range(warmup + reps):
        t = time.perf_counter()
        hits, ptr, ops = e.ualign_run(unit, bases, off)
        wall = (time.perf_counter() - t) * 1e3
        if rep >= warmup:
            runs.append(dict(e.ualign_info()["phase_ms"], wall_ms=wall))
    info = e.ualign_info()
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    lens = np.diff(off)
    score_cells = 2 * int(lens.sum()) * len(unit)
    move_cells = int(hits["r_en"].astype(np.int64).sum()) * len(unit)
    share = (hits["r_en"] - hits["r_st"]) / np.maximum(lens, 1)
    out = {"reads": int(n_reads), "bases": int(lens.sum()), "unit_len": len(unit), "reps": reps, "phase_ms_median": med, "phase_ms_runs": runs,
           "score_pass_cells": score_cells, "moves_pass_cells": move_cells, "score_pass_cells_per_s": score_cells / (med["score"] * 1e-3),
           "moves_pass_cells_per_s": move_cells / (med["moves"] * 1e-3), "cells_per_s_of_the_call": (score_cells + move_cells) / (med["total"] * 1e-3),
           "reads_with_a_hit": int(hits["status"].sum()), "minus_strand_hits": int(hits["strand"].sum()),
           "share_of_bases_inside_the_interval": {"mean": float(share.mean()), "min": float(share.min()), "median": float(np.median(share))},
           "op_columns": int(ops.size), "n_batches": info["n_batches"], "batch_bytes": info["batch_bytes"], "launch_cap": info["launch_cap"]}
    # (b) the restatement on one host core over the first reads, scaled by cells
    t = time.perf_counter()
    cells = 0
    for q in range(min(sample, n_reads)):
        r = bases[off[q]:off[q + 1]].tobytes()
        w = uc.align_np(unit, r)
        assert uc.same(hits[q], ops[ptr[q]:ptr[q + 1]], w), f"read {q} differs from the restatement"
        cells += 2 * len(r) * len(unit)
    secs = time.perf_counter() - t
    out["restatement_one_core"] = {"reads": min(sample, n_reads), "cells": cells, "seconds": secs, "cells_per_s": cells / secs,
                                   "SCALED_to_all_reads_seconds": secs * score_cells / max(cells, 1),
                                   "note": "numpy restatement of the rule (tests/ualigncheck.py align_np), one core, both strands, walk included; scaled by score-pass cells; "
                                           "NOT a figure of NCRF, which is not available"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, action="append", default=None, help="reads of the benchmark's generator (repeatable; default 500 and 50000)")
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=3, help="reads the restatement is run on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "tools/ualign_wall.py", "scores": {"match": 10, "mismatch": 35, "gap": 33}, "runs": []}
    with Engine(0) as e:
        res["device"] = e.device_info()
        for n in a.reads or [500, 50000]:
            res["runs"].append(measure(e, n, a.seed, a.reps, a.warmup, a.sample))
            print(json.dumps({k: v for k, v in res["runs"][-1].items() if k != "phase_ms_runs"}), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()

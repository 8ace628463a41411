#!/usr/bin/env python3
"""Device time of the built-in monomer decomposer (cf_monodec_run) on D6Z1-shaped reads, and what there is to compare
it with.

  (a) --reads reads of --length bases each (50 000 x 20 000 is the cen6 workload's order; 500 is the short run): the 18 D6Z1 monomers
      (tests/golden/D6Z1_monomers.fasta, 3 065 bases) in HOR order read cyclically from a random phase, with the generator's error
      rates (2 % substitutions, 2 % insertions, 1.5 % deletions), every second read reverse-complemented.  Device ms per phase by
      HIP events (cf_monodec_info), the wall time of the call, cells per second (2 strands x read bytes x 3 065 columns per score
      pass; read bytes x 3 065 per moves pass), instances, the share of '?' instances at --min-identity 69;
  (b) there is no String Decomposer figure: the only comparison is the rule's numpy restatement (tests/monodeccheck.py) on one host
      core over the first --sample reads cut to --sample-length bases, SCALED by cells to all reads and labelled as scaled; the
      device's answer for those reads is checked against it on the way.

    python tools/monodec_wall.py --reads 500 --reads 50000 --out profiles/r27_monodec.json
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
import monodeccheck as mc  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

_COMP = np.zeros(256, np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")
SUB, INS, DEL = 0.02, 0.02, 0.015


def reads_of(hor, n_reads, length, seed, chunk=2000):
    """(bases uint8, read_off int64): vectorised over chunks of reads"""
    rng = np.random.default_rng(seed)
    hor = np.frombuffer(hor, np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts, lens = [], []
    for lo in range(0, n_reads, chunk):
        R = min(chunk, n_reads - lo)
        idx = (rng.integers(0, hor.size, R)[:, None] + np.arange(length)[None, :]) % hor.size
        b = hor[idx].ravel()
        p = rng.random(b.size, dtype=np.float32)
        rnd = acgt[rng.integers(0, 4, b.size, dtype=np.uint8)]
        sub = (p >= DEL) & (p < DEL + SUB)
        b = np.where(sub, rnd, b)
        rep = (p >= DEL).astype(np.int8) + ((p >= DEL + SUB) & (p < DEL + SUB + INS))
        flat = np.repeat(b, rep)
        ins_pos = np.cumsum(rep, dtype=np.int64)[rep == 2] - 2
        flat[ins_pos] = acgt[rng.integers(0, 4, ins_pos.size, dtype=np.uint8)]
        parts.append(flat)
        lens.append(rep.reshape(R, length).sum(1, dtype=np.int64))
    bases = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    for q in range(1, n_reads, 2):
        bases[off[q]:off[q + 1]] = _COMP[bases[off[q]:off[q + 1]]][::-1]
    return bases, off


def measure(e, seqs, n_reads, length, seed, reps, warmup, sample, sample_length):
    L = sum(len(s) for s in seqs)
    bases, off = reads_of(b"".join(seqs), n_reads, length, seed)
    runs = []
    for rep in range(warmup + reps):
        t = time.perf_counter()
        info, ptr, inst = e.monodec(seqs, bases, off)
        wall = (time.perf_counter() - t) * 1e3
        if rep >= warmup:
            runs.append(dict(e.monodec_info()["phase_ms"], wall_ms=wall))
    shape = e.monodec_info()
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    n_bases = int(off[-1])
    score_cells, move_cells = 2 * n_bases * L, n_bases * L
    cols = (inst["n_match"].astype(np.int64) + inst["n_mismatch"] + inst["n_ins"] + inst["n_del"])
    out = {"reads": int(n_reads), "bases": n_bases, "columns": L, "monomers": len(seqs), "reps": reps, "phase_ms_median": med, "phase_ms_runs": runs,
           "score_pass_cells": score_cells, "moves_pass_cells": move_cells, "score_pass_cells_per_s": score_cells / (med["score"] * 1e-3),
           "moves_pass_cells_per_s": move_cells / (med["moves"] * 1e-3), "cells_per_s_of_the_call": (score_cells + move_cells) / (med["total"] * 1e-3),
           "cells_per_s_of_the_wall_time": (score_cells + move_cells) / (med["wall_ms"] * 1e-3),
           "instances": int(inst.size), "minus_strand_reads": int(info["strand"].sum()), "reads_with_a_prefix": int((info["prefix"] > 0).sum()),
           "unsure_instances_at_69": int((100 * inst["n_match"].astype(np.int64) < 69 * cols).sum()),
           "n_batches": shape["n_batches"], "batch_bytes": shape["batch_bytes"], "launch_cap": shape["launch_cap"]}
    # (b) the restatement on one host core over the first reads (cut short), scaled by cells
    if sample:
        cut = [bases[off[q]:off[q + 1]][:sample_length].tobytes() for q in range(min(sample, n_reads))]
        t = time.perf_counter()
        wants = [mc.decompose_np(seqs, r) for r in cut]
        secs = time.perf_counter() - t
        mc.check(e, seqs, cut, wants=wants)
        cells = 2 * sum(len(r) for r in cut) * L
        out["restatement_one_core"] = {"reads": len(cut), "cells": cells, "seconds": secs, "cells_per_s": cells / secs,
                                       "SCALED_to_all_reads_seconds": secs * score_cells / max(cells, 1),
                                       "note": "numpy restatement of the rule (tests/monodeccheck.py decompose_np), one core, both strands, moves pass and walk "
                                               "included; scaled by score-pass cells; NOT a figure of String Decomposer, which is not available"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, action="append", default=None, help="reads (repeatable; default 500 and 50000)")
    ap.add_argument("--length", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=2, help="reads the restatement is run on")
    ap.add_argument("--sample-length", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seqs = [s for _, s in mc.d6z1_monomers()]
    res = {"tool": "tools/monodec_wall.py", "scores": {"match": 1, "mismatch": 1, "gap": 1}, "error_rates": {"sub": SUB, "ins": INS, "del": DEL}, "runs": []}
    with Engine(0) as e:
        res["device"] = e.device_info()
        for n in a.reads or [500, 50000]:
            res["runs"].append(measure(e, seqs, n, a.length, a.seed, a.reps, a.warmup, a.sample, a.sample_length))
            print(json.dumps({k: v for k, v in res["runs"][-1].items() if k != "phase_ms_runs"}), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()

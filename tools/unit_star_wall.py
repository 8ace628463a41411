#!/usr/bin/env python3
"""Wall time of stage 4 (scripts/better_consensus_unit_reconstruction.py) by phase on one GPU: parse, load, count, top n, graph,
alignment, write — on a synthetic report of the bench's workload (bench.synth_kwargs), --unit = the generator's motif rotated by 37
with three substitutions.  Prints one JSON record (profiles/r08_unit_star_cli.json).

    python tools/unit_star_wall.py --reads 50000 --k 30 --out unit_star_cli.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    from centroflye_amd import _host, session
    from centroflye_amd import better_consensus_unit_reconstruction as B
    with tempfile.TemporaryDirectory() as wd:
        rpt = os.path.join(wd, "reads.ncrf")
        t = time.perf_counter()
        _host.synth(report_path=rpt, pack=False, n_reads=a.reads, **bench.synth_kwargs(a.reads, a.seed))
        t_synth = time.perf_counter() - t
        pk = _host.parse_report(rpt, keep_rows=False)
        motif = pk.motifs[int(pk.meta[0][7])]
        n_bases = int(pk.n_bases)
        del pk
        u = list(motif[37:] + motif[:37])
        for p in (100, 1000, 2000):
            u[p % len(u)] = "A" if u[p % len(u)] != "A" else "C"
        unit_fn = os.path.join(wd, "unit.fasta")
        with open(unit_fn, "w") as f:
            f.write(">unit\n" + "".join(u) + "\n")
        runs = []
        for r in range(a.repeats):
            session.reset()                     # every run starts as a fresh process would: a new device context
            times = {}
            t = time.perf_counter()
            got, st = B.run(B.parse_args(["--reads-ncrf", rpt, "--unit", unit_fn, "-k", str(a.k),
                                          "--output", os.path.join(wd, f"out{r}", "unit_star.fasta")]), times)
            times["total"] = time.perf_counter() - t
            runs.append(dict({k: round(v, 4) for k, v in times.items()}, graph_stats=st,
                             unit_star_is_rotated_motif=got == motif[37:] + motif[:37]))
        session.reset()
    rec = dict(what="stage 4 CLI wall time by phase (seconds), one MI355X", reads=a.reads, seed=a.seed, k=a.k, n_bases=n_bases,
               report_bytes_synth_s=round(t_synth, 2), unit_len=len(motif), n_top=B.n_top("".join(u), a.k), runs=runs,
               note="run 0 includes the device context's first use; parse = unit FASTA + NCRF report text to packed arrays")
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

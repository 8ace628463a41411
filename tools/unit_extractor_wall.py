#!/usr/bin/env python3
"""Device and wall time of the unit extractor (cf_tandem.hip + centroflye_amd/unit_extractor.py) on the benchmark's own
reads: the 50 000 synthetic DXZ1-HOR reads of bench.py (the de-gapped rows of the generator, ~1 Gb), k = 15, bin size 10.

  device   cf_tandem_scan on all reads: HIP-event milliseconds per phase (records, sorts, runs and distances, windows, hook) and of
           the whole call with its copies, the median of --reps runs after --warmup
  wall     extract_units on the same reads as a FASTA file, without and with writing the two files per read and periods.tsv
  host     the reference-rule host functions of the mirror module (what the reference does per read) on ONE core, on a fixed
           sample of --sample of those reads in the same run, compared with the device's answers and SCALED to the whole set

    python tools/unit_extractor_wall.py --out profiles/r13_unit_extractor.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centroflye_amd import _host, _lib, unit_extractor as ue  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

PHASES = ("records", "sorts", "runs", "windows", "hook", "total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("-k", type=int, default=15)
    ap.add_argument("--bin-size", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--no-files", action="store_true", help="skip the extract_units legs")
    ap.add_argument("--param", action="append", default=[], help="library knob name=value (cf_set_param)")
    ap.add_argument("--lib", default=None, help="test hook: another build of libcfhip (the host-emulated one, to try this tool without a GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pk = _host.synth(n_reads=a.reads, seed=a.seed, n_units=max(24, int(round(0.3 * a.reads))), var_len=8)      # bench.py's workload
    bases, off = np.ascontiguousarray(pk.bases), np.ascontiguousarray(pk.read_off)
    n = off.size - 1
    res = dict(workload=f"{n} reads / {int(off[-1])} bases (bench.py: seed {a.seed}, var_len 8), k = {a.k}, bin size {a.bin_size}", reps=a.reps,
               warmup=a.warmup)
    with Engine(0, _lib.load(a.lib) if a.lib else None) as e:
        res["device"] = e.device_info()["name"]
        for kv in a.param:
            name, value = kv.split("=")
            e.set_param(name, int(value))
        runs, walls = [], []
        for i in range(a.warmup + a.reps):
            t = time.perf_counter()
            rows = e.tandem_scan(bases, off, a.k, a.bin_size)
            walls.append((time.perf_counter() - t) * 1e3)
            runs.append(e.tandem_info()["phase_ms"])
        info = e.tandem_info()
        ptr, pos = e.tandem_hook_positions()
        res["shape"] = {f: info[f] for f in ("batch_windows", "key_mode", "code_bits", "read_bits", "pos_bits", "pos_shift", "n_batches", "n_key_batches", "n_records")}
        res["device_ms"] = {p: statistics.median(r[p] for r in runs[a.warmup:]) for p in PHASES}
        res["device_ms_runs"] = {p: [round(r[p], 3) for r in runs[a.warmup:]] for p in PHASES}
        res["scan_wall_ms"] = statistics.median(walls[a.warmup:])
        sort_keys = info["n_records"] + int(rows["n_conv"].sum())
        res["sort_ns_per_record"] = res["device_ms"]["sorts"] * 1e6 / max(sort_keys, 1)
        res["status_counts"] = {s: int((rows["status"] == i).sum()) for i, s in enumerate(ue.STATUS)}
        ok = rows["status"] == 0
        res["period_median"] = float(np.median(rows["period"][ok])) if ok.any() else None
        res["n_distances"] = int(rows["n_conv"].sum())
        res["n_hook_positions"] = int(pos.size)
        # the reference's rules on one core, a fixed sample
        sample = np.unique(np.linspace(0, n - 1, min(a.sample, n)).astype(np.int64))
        same, secs = 0, 0.0
        for i in sample:
            seq = bases[off[i]:off[i + 1]].tobytes().decode("latin-1")
            t = time.perf_counter()
            h = ue.scan_read_on_host(str(i), seq, a.k, a.bin_size)
            secs += time.perf_counter() - t
            r = rows[i]
            if r["status"] == 2:
                same += 1      # (redone on the host anyway)
            elif h.status == "no_period":
                same += int(r["status"] == 1)
            else:
                same += int((h.period, h.count, h.bin_left, h.bin_right, h.hook_index, h.hook_pos) ==
                            (r["period"], r["count"], r["bin_left"], r["bin_right"], r["hook_index"], pos[ptr[i]:ptr[i + 1]].tolist()))
        sample_bases = int(sum(off[i + 1] - off[i] for i in sample))
        res["host_one_core"] = dict(sample_reads=int(sample.size), sample_bases=sample_bases, sample_secs=secs, sample_matches_device=int(same),
                                    scaled_secs_whole_set=secs * float(off[-1]) / max(sample_bases, 1), extrapolated=True,
                                    note="scaled by bases from the sample to the whole set; the functions are the mirror module's host statements of the reference's rules")
        if not a.no_files:
            tmp = tempfile.mkdtemp(prefix="unit_extractor_wall_")
            try:
                fa = os.path.join(tmp, "reads.fasta")
                with open(fa, "wb") as f:
                    for i in range(n):
                        f.write(b">r%06d\n" % i)
                        f.write(bases[off[i]:off[i + 1]].tobytes())
                        f.write(b"\n")
                for key, write in (("extract_units_wall_s_no_files", False), ("extract_units_wall_s_with_files", True)):
                    t = time.perf_counter()
                    out_rows = ue.extract_units(fa, os.path.join(tmp, "out"), a.k, a.bin_size, engine=e, write_files=write)
                    res[key] = time.perf_counter() - t
                res["reads_with_files"] = sum(r["status"] == "ok" for r in out_rows)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

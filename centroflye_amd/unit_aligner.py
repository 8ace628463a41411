"""Stage 1: reads + HOR unit -> ``<outdir>/report.ncrf``, the file every later stage starts from.

Counterpart of the reference's ``scripts/run_ncrf_parallel.py`` (same flags: --reads, --repeat, -t/--threads, -o/--outdir,
--ncrf-bin), which cuts the reads into chunks and starts one external ``NCRF unit:<seq>`` process per chunk (:49-62), joins
their reports without the end-of-file lines (:64-70) and writes the unit's sequence for the word "unit" (:72-73).

``--aligner ncrf`` (the default) does the same with the external binary.  ``--aligner builtin`` needs no external program: the
library's own tandem aligner (``cf_ualign_run``, include/cfhip.h: local alignment with linear gaps of every read against the unit
read cyclically, both strands, on the GPU) gives the best stretch of every read, and the host library writes the records.  The
built-in aligner is NOT NCRF: its scoring (--match / --mismatch / --gap) is its own, it reports at most one record per read,
and it does not claim NCRF's output.  Records shorter than --min-length read bases are not written.
"""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np

from .read_recruitment import iter_seqs, read_first_seq

BATCH_BASES = 1 << 30


def header_line(match, mismatch, gap):
    return f"# aligner=builtin match={match} mismatch={mismatch} gap={gap}\n"


def run_builtin(unit, reads_path, report_path, match=10, mismatch=35, gap=33, min_length=500, engine=None):
    """Writes report_path; returns (reads seen, records written)."""
    from . import _host, session
    engine = engine or session.engine()
    n_seen = n_written = 0
    part = report_path + ".part"
    batch, size, first = [], 0, True

    def flush():
        nonlocal batch, size, first, n_written
        off = np.zeros(len(batch) + 1, np.int64)
        np.cumsum([len(s) for _, s in batch], out=off[1:])
        flat = np.frombuffer(b"".join(s for _, s in batch), dtype=np.uint8)
        hits, op_ptr, ops = engine.ualign_run(unit, flat, off, match, mismatch, gap)
        n_written += _host.write_ualign_report(part, header_line(match, mismatch, gap) if first else None, unit, [n for n, _ in batch], flat, off,
                                               hits, op_ptr, ops, min_length)
        with open(report_path, "ab") as out, open(part, "rb") as f:
            shutil.copyfileobj(f, out)
        os.remove(part)
        batch, size, first = [], 0, False

    open(report_path, "wb").close()
    for name, seq in iter_seqs(reads_path):
        batch.append((name, seq))
        size += len(seq)
        n_seen += 1
        if size >= BATCH_BASES:
            flush()
    if batch or first:
        flush()
    return n_seen, n_written


def run_ncrf(unit, reads_path, outdir, threads, ncrf_bin):
    """One NCRF process per chunk of reads, as run_ncrf_parallel.py:36-73 does."""
    reads = list(iter_seqs(reads_path))
    n_chunks = max(1, min(int(threads), len(reads)))
    split_dir, rep_dir = os.path.join(outdir, "split_reads"), os.path.join(outdir, "ncrf_report")
    os.makedirs(split_dir, exist_ok=True)
    os.makedirs(rep_dir, exist_ok=True)
    procs, reports = [], []
    for c in range(n_chunks):
        fn = os.path.join(split_dir, f"split_reads_{c}.fasta")
        with open(fn, "wb") as f:
            for name, seq in reads[c::n_chunks]:
                f.write(b">" + name + b"\n" + seq + b"\n")
        rep = os.path.join(rep_dir, f"report_{c}.ncrf")
        reports.append(rep)
        with open(fn, "rb") as fin, open(rep, "wb") as fout:
            procs.append(subprocess.Popen([ncrf_bin, "unit:" + unit.decode()], stdin=fin, stdout=fout))
    bad = [p.args[0] for p in procs if p.wait() != 0]
    if bad:
        raise RuntimeError(f"{bad[0]} failed on {len(bad)} of {len(procs)} chunks")
    with open(os.path.join(outdir, "report.ncrf"), "wb") as out:
        for rep in reports:
            with open(rep, "rb") as f:
                for line in f:
                    if b"end-of-file" not in line:
                        out.write(line.replace(b"unit", unit))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", required=True, help="Path to centromeric reads (FASTA or FASTQ, plain or gzip)")
    ap.add_argument("--repeat", required=True, help="Path to the unit sequence")
    ap.add_argument("-t", "--threads", type=int, default=30, help="Number of NCRF processes (--aligner ncrf)")
    ap.add_argument("-o", "--outdir", required=True, help="Output directory")
    ap.add_argument("--ncrf-bin", default="NCRF", help="Path to binary of NCRF")
    ap.add_argument("--aligner", choices=("ncrf", "builtin"), default="ncrf",
                    help="ncrf: the external binary, as the reference; builtin: the library's own tandem aligner on the GPU (not NCRF's output)")
    ap.add_argument("--match", type=int, default=10, help="builtin: score of a match")
    ap.add_argument("--mismatch", type=int, default=35, help="builtin: penalty of a mismatch")
    ap.add_argument("--gap", type=int, default=33, help="builtin: penalty of a gap column")
    ap.add_argument("--min-length", type=int, default=500, help="builtin: records of fewer aligned read bases are not written")
    params = ap.parse_args(argv)
    unit = read_first_seq(params.repeat)
    report_fn = os.path.join(params.outdir, "report.ncrf")
    if params.aligner == "ncrf":
        if shutil.which(params.ncrf_bin) is None:
            sys.exit(f"run_ncrf_parallel.py: the NCRF binary '{params.ncrf_bin}' was not found (--ncrf-bin; or --aligner builtin, which needs none)")
        os.makedirs(params.outdir, exist_ok=True)
        run_ncrf(unit, params.reads, params.outdir, params.threads, params.ncrf_bin)
        return 0
    from .engine import DeviceError
    os.makedirs(params.outdir, exist_ok=True)
    try:
        n_seen, n_written = run_builtin(unit.upper(), params.reads, report_fn, params.match, params.mismatch, params.gap, params.min_length)
    except DeviceError as e:
        if os.path.exists(report_fn):
            os.remove(report_fn)
        sys.exit(f"run_ncrf_parallel.py: {e}")
    print(f"{n_written} records of {n_seen} reads written to {report_fn}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

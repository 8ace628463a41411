"""Reads + monomers -> ``decomposition.tsv``, the report the monostring parser (``sd_parser``) starts from.

The reference's second pipeline (``run_all_cen6.sh``, ``scripts/centroFlyeMono.py``) takes this report from String Decomposer, an
external program.  Here the library's own monomer decomposer (``cf_monodec_run``, include/cfhip.h) writes it: every read is cut
into a chain of monomer instances by one dynamic program against all monomers at once (global alignment with linear gaps, both
strands, on the GPU), and the host library writes one line per instance in the six columns ``sd_parser.py:174-180`` names: read id,
monomer name (with an apostrophe on the '-' strand), first and last read base, identity ("%.2f" of 100 matches / alignment
columns) and reliability ('+' iff the identity reaches --min-identity, else '?').  The built-in decomposer is NOT String
Decomposer: its rule and scoring (--match / --mismatch / --gap) are its own and it does not claim String Decomposer's output
(DESIGN §27).  The unassigned bases in front of a read's first instance get no line.
"""
import argparse
import os
import sys

import numpy as np

from .read_recruitment import iter_seqs

BATCH_BASES = 1 << 30


def read_monomers(path):
    """[(name, upper-case sequence)] in file order; the name is the FASTA id up to the first blank"""
    return [(name, seq.upper()) for name, seq in iter_seqs(path)]


def run(monomers, reads_path, out_path, match=1, mismatch=1, gap=1, min_identity=69, engine=None):
    """Writes out_path (through out_path + '.tmp' and a rename); returns (reads seen, lines written)."""
    from . import _host, session
    engine = engine or session.engine()
    names = [n for n, _ in monomers]
    seqs = [s for _, s in monomers]
    tmp, part = out_path + ".tmp", out_path + ".part"
    n_seen = n_lines = 0
    batch, size = [], 0

    def flush(out):
        nonlocal batch, size, n_lines
        off = np.zeros(len(batch) + 1, np.int64)
        np.cumsum([len(s) for _, s in batch], out=off[1:])
        flat = np.frombuffer(b"".join(s for _, s in batch), dtype=np.uint8)
        info, ptr, inst = engine.monodec(seqs, flat, off, match, mismatch, gap)
        n_lines += _host.write_sd_report(part, [n for n, _ in batch], names, info, ptr, inst, min_identity)
        with open(part, "rb") as f:
            while True:
                blk = f.read(1 << 24)
                if not blk:
                    break
                out.write(blk)
        os.remove(part)
        batch, size = [], 0

    try:
        with open(tmp, "wb") as out:
            for name, seq in iter_seqs(reads_path):
                batch.append((name, seq))
                size += len(seq)
                n_seen += 1
                if size >= BATCH_BASES:
                    flush(out)
            flush(out)      # (an empty last batch still asks the library to look at the monomers and the scores)
        os.replace(tmp, out_path)
    finally:
        for fn in (tmp, part, part + ".tmp"):
            if os.path.exists(fn):
                os.remove(fn)
    return n_seen, n_lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--sequences", required=True, help="Path to the reads (FASTA or FASTQ, plain or gzip)")
    ap.add_argument("-m", "--monomers", required=True, help="FASTA with the monomers")
    ap.add_argument("-o", "--out-file", default="decomposition.tsv", help="The report (default decomposition.tsv)")
    ap.add_argument("--match", type=int, default=1, help="score of a match")
    ap.add_argument("--mismatch", type=int, default=1, help="penalty of a mismatch")
    ap.add_argument("--gap", type=int, default=1, help="penalty of a gap column")
    ap.add_argument("--min-identity", type=int, default=69, help="instances of a lower identity (in percent) are marked '?'")
    ap.add_argument("-t", "--threads", type=int, default=1, help="accepted and ignored (the work runs on the GPU)")
    params = ap.parse_args(argv)
    from .engine import DeviceError
    try:
        monomers = read_monomers(params.monomers)
        n_seen, n_lines = run(monomers, params.sequences, params.out_file, params.match, params.mismatch, params.gap, params.min_identity)
    except (DeviceError, OSError, ValueError) as e:
        sys.exit(f"monomer_decomposer.py: {e}")
    print(f"{n_lines} monomer instances of {n_seen} reads written to {params.out_file}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

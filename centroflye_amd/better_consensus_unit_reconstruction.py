"""Drop-in counterpart of the reference's ``scripts/better_consensus_unit_reconstruction.py`` (stage 4, centroFlye.py:212-225):
same function names, signatures and CLI.

  get_kmer_counts_reads (:129-137), get_most_frequent_kmers (:156-167)  k-mer occurrence counts and the top n on the GPU
      (cf_count_occurrences, cf_top_kmers)
  get_polished_unit (:170-190)  the de Bruijn purification and the edlib re-phasing in the host library (cfh_unit_star)
  parse_args (:140-153), main (:193-212)

The CLI never pulls the count table to the host: it takes the top n keys and counts from the device and adds the few windows
that hold a symbol other than upper-case A, C, G, T (the device skips them; the reference counts them as k-mers of their own) from
the host scan.  The top n go into the graph in descending (count, k-mer) order — the order heapq.nlargest returns before the
reference turns it into a set whose iteration order depends on PYTHONHASHSEED.  DeBruijnGraph and get_coverage,
which return networkx objects in the reference, are not mirrored.
"""
import argparse
import os
import sys
import time
from collections.abc import Sequence

import numpy as np

from . import _host
from . import kmers as km
from . import session

MAX_K = 31      # device keys are 2-bit codes in 64 bits


def get_kmer_counts_reads(ncrf_report, k=19):
    """kmer -> number of occurrences over all (de-gapped) read rows."""
    e = session.ensure_loaded(ncrf_report.packed, 1)
    e.count_occurrences(k)
    keys, lo, hi = e.table()
    return km.KmerFreqs(keys, lo.astype(np.int64) | (hi.astype(np.int64) << 32), k)


def get_most_frequent_kmers(reads_ncrf_report, k, unit_seq):
    """(counts mapping, set of the 3 * |unit k-mers| most frequent k-mers by (count, k-mer))."""
    unit_double_seq = unit_seq + unit_seq
    n_unit_kmers = len({unit_double_seq[i:i + k] for i in range(len(unit_seq))})
    kmer_counts_reads = get_kmer_counts_reads(reads_ncrf_report, k=k)
    keys, _ = session.engine().top_kmers(int(n_unit_kmers * 3))
    return kmer_counts_reads, set(km.decode(keys, k))


def get_polished_unit(k, most_frequent_kmers, kmer_counts_reads, unit_seq):
    """The unit* string.  A list or tuple of k-mers enters the graph in its own order, as in the reference; any other collection
    (the reference passes a set) in descending (count, k-mer) order.  Raises _host.UnitStarError where the reference raises."""
    kms = list(most_frequent_kmers)
    if not isinstance(most_frequent_kmers, Sequence):
        kms.sort(key=lambda s: (kmer_counts_reads[s], s), reverse=True)
    return _host.unit_star(k, kms, [kmer_counts_reads[s] for s in kms], unit_seq)[0]


def n_top(unit_seq, k):
    """n of the reference (:158-163): three times the distinct k-long windows of the doubled unit that start in its first copy."""
    dbl = unit_seq + unit_seq
    return int(len({dbl[i:i + k] for i in range(len(unit_seq))}) * 3)


def read_unit(path):
    """The reference's read_bio_seq (utils/bio.py:11-24) for the formats this stage accepts: the extension decides (fasta, fa,
    fna; anything else is refused, as Biopython refuses it); the first record's id, and the LAST record with that id (the
    reference builds {id: seq}); sequence lines right-stripped, joined, spaces and CRs dropped, letter case kept."""
    ext = path.split(".")[-1]
    if ext not in ("fasta", "fa", "fna"):
        raise ValueError(f"{path}: unit files must be FASTA (.fasta, .fa or .fna), not '{ext}'")
    recs = []
    with open(path) as f:
        title, lines = None, []
        for ln in f:
            if ln[:1] == ">":
                if title is not None:
                    recs.append((title, lines))
                title, lines = ln[1:].rstrip(), []
            elif title is not None:
                lines.append(ln.rstrip())
        if title is not None:
            recs.append((title, lines))
    if not recs:
        raise ValueError(f"{path}: no FASTA record")
    ids = [(t.split(None, 1) or [""])[0] for t, _ in recs]
    last = max(i for i, x in enumerate(ids) if x == ids[0])
    return "".join(recs[last][1]).replace(" ", "").replace("\r", "")


def top_kmers(packed, k, n, times=None):
    """[k-mer], [count] of the n k-mers with the largest (count, k-mer), descending — heapq.nlargest over every window of the
    de-gapped rows.  Device top n, merged with the host's windows that the device does not count."""
    t = time.perf_counter()
    e = session.ensure_loaded(packed, 1)
    t = _tick(times, "load", t)
    with e.knobs(count_skip_exotic=1):
        e.count_occurrences(k)
    t = _tick(times, "count", t)
    keys, counts = e.top_kmers(n)
    strs, cnts = km.decode(keys, k) if keys.size else [], [int(c) for c in counts]
    if packed.non_acgt and n > 0:
        extra = packed.exotic_occurrences(k, cnts[-1] if len(strs) >= n else 1)
        if extra:
            merged = sorted(list(zip(strs, cnts)) + extra, key=lambda x: (x[1], x[0]), reverse=True)[:n]
            strs, cnts = [x[0] for x in merged], [x[1] for x in merged]
    _tick(times, "top_n", t)
    return strs, cnts


def _tick(times, name, t0):
    t1 = time.perf_counter()
    if times is not None:
        times[name] = times.get(name, 0.0) + (t1 - t0)
    return t1


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--reads-ncrf", help="NCRF report on centromeric reads", required=True)
    parser.add_argument("--unit", help="Initial unit sequence of centromeric read", required=True)
    parser.add_argument("-k", type=int, default=30)
    parser.add_argument("--output", help="Output file for polished unit", required=True)
    return parser.parse_args(argv)


def run(params, times=None):
    """The stage on parsed arguments; returns (unit*, graph stats).  times (dict, optional) gets the seconds of each phase."""
    if not 2 <= params.k <= MAX_K:
        raise ValueError(f"-k {params.k}: this stage supports 2 <= k <= {MAX_K} (k-mers are counted as 2-bit codes in 64 bits)")
    t = time.perf_counter()
    outdir = os.path.dirname(params.output)
    if outdir:
        os.makedirs(outdir, exist_ok=True)
    unit_seq = read_unit(params.unit)
    packed = _host.parse_report(params.reads_ncrf, keep_rows=False)
    t = _tick(times, "parse", t)
    strs, cnts = top_kmers(packed, params.k, n_top(unit_seq, params.k), times)
    unit_star, st = _host.unit_star(params.k, strs, cnts, unit_seq)
    if times is not None:
        times["graph"] = st["graph_us"] * 1e-6
        times["alignment"] = st["align_us"] * 1e-6
    t = time.perf_counter()
    tmp = params.output + ".tmp"
    with open(tmp, "w") as f:
        f.write(f">unit*\n{unit_star}\n")          # utils/bio.py:32-36 write_bio_seqs
    os.replace(tmp, params.output)
    _tick(times, "write", t)
    return unit_star, st


def main(argv=None):
    params = parse_args(argv)
    try:
        run(params)
    except (ValueError, OSError, _host.HostError) as e:
        sys.exit(f"better_consensus_unit_reconstruction: {e}")


if __name__ == "__main__":
    main()

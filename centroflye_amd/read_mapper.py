"""Batch mapping of reads onto a finished cloud contig: the reference's ``map_reads_fast``
(scripts/cloud_contig.py:117-156) on the GPU.

The greedy placer writes ``r_id None`` for every read that did not pass its thresholds at the moment it was picked
(read_placer.py:63-94).  The reference can ask afterwards where such a read belongs on the FINISHED contig — build a
``CloudContig`` from the placed reads (``add_read``, cloud_contig.py:26-41) and call ``map_reads_fast`` — but only on Python
dicts.  Here the contig is built by one sort (``cf_contig_build``) and every query read is scored by one kernel
(``cf_map_reads``); there is no dependency between reads.

``map_reads_fast`` below keeps the reference's return value, positions of the mapped reads only; ``ReadMapper`` is the
command line (scripts/map_reads.py), which writes ``mapped_positions.csv``.

``map_reads_fast`` seeds from every position of a frequent k-mer.  The reference's ground truth is the exact scorer,
``CloudContig.calc_inters_score`` (:46-76), which counts at a position only the k-mers that are frequent THERE; ``map_reads``
(:98-114) is built on it and ``map_reads_fast(debug=True)`` (:146-155) cross-checks against it.  ``calc_inters_score`` and
``map_reads`` below run it for a batch of reads in one kernel (``cf_score_reads``).
"""
import argparse
import os

import numpy as np

from . import _host
from . import kmers as km
from .ncrf_parser import NCRF_Report
from .read_kmer_cloud import filter_reads_kmer_clouds, get_reads_kmer_clouds


def backbone_of(read_placement, ids):
    """(read indices, positions) of the placed reads.  read_placement: {r_id: position or None} as
    eltr_polisher.read_reported_positions returns it, or the (read, pos, s0, s1) arrays of ReadPlacer.run()."""
    if isinstance(read_placement, dict):
        row = {r_id: i for i, r_id in enumerate(ids)}
        items = [(row[r_id], p) for r_id, p in read_placement.items() if p is not None]
        reads = np.array([r for r, _ in items], np.int64)
        pos = np.array([p for _, p in items], np.int64)
    else:
        reads = np.asarray(read_placement[0], np.int64)
        pos = np.asarray(read_placement[1], np.int64)
        reads, pos = reads[pos >= 0], pos[pos >= 0]
    return reads, pos


def _contig_and_query(read_placement, reads_kmer_clouds, min_cloud_kmer_freq, reads):
    """Builds the contig of the placed reads; (engine, ids, row indices of the query reads)."""
    ids = reads_kmer_clouds.report.packed.ids
    engine = reads_kmer_clouds.on_device()
    b_reads, b_pos = backbone_of(read_placement, ids)
    engine.contig_build(b_reads, b_pos, min_cloud_kmer_freq)
    if reads is None:
        query = np.arange(len(ids), dtype=np.int64)
    else:
        row = {r_id: i for i, r_id in enumerate(ids)}
        query = np.array([row[r_id] for r_id in reads], np.int64)
    return engine, ids, query


def map_reads_fast(read_placement, reads_kmer_clouds, min_cloud_kmer_freq=2, threshold=(5, 10), reads=None, debug=False):
    """({r_id: position}, {r_id: (s0, s1)}) of the reads that map onto the contig of the placed reads of ``read_placement``
    (cloud_contig.py:117-156 after CloudContig.add_read of every placed read).  reads_kmer_clouds: the KMerClouds of
    read_kmer_cloud.get_reads_kmer_clouds / filter_reads_kmer_clouds; reads: the r_ids to map (default: all).
    debug=True (:146-155): a third value, the list (r_id, fast_score, exact_score, fast_pos, exact_pos) of the mapped reads whose
    exact answer over [0, max_pos - units + 1] under the same thresholds differs in score or position (exact_pos None when no
    start qualifies) — what the reference prints."""
    engine, ids, query = _contig_and_query(read_placement, reads_kmer_clouds, min_cloud_kmer_freq, reads)
    pos, s0, s1 = engine.map_reads(query, threshold)
    positions, scores = {}, {}
    for r, p, a, b in zip(query.tolist(), pos.tolist(), s0.tolist(), s1.tolist()):
        if p >= 0:
            positions[ids[r]] = p
            scores[ids[r]] = (a, b)
    if not debug:
        return positions, scores
    mapped = pos >= 0
    xp, x0, x1 = engine.score_reads(query[mapped], None, None, threshold[0], threshold[1])
    differ = (xp != pos[mapped]) | (x0 != s0[mapped]) | (x1 != s1[mapped])
    disagreements = [(ids[r], (a, b), (c, d), p, (xq if xq >= 0 else None))
                     for r, p, a, b, xq, c, d in zip(query[mapped][differ].tolist(), pos[mapped][differ].tolist(), s0[mapped][differ].tolist(),
                                                     s1[mapped][differ].tolist(), xp[differ].tolist(), x0[differ].tolist(), x1[differ].tolist())]
    return positions, scores, disagreements


def calc_inters_score(read_placement, reads_kmer_clouds, min_cloud_kmer_freq=2, reads=None, min_position=0, max_position=None,
                      min_unit=2, min_inters=10):
    """{r_id: ((s0, s1), position or None)}: CloudContig.calc_inters_score (cloud_contig.py:46-76) of every query read on the
    contig of the placed reads.  min_position / max_position: one value for all reads or one per query read; max_position None is
    map_reads' range, max_pos - units + 1 (the reference's own default, max_pos, is ``engine.contig_info()["max_pos"]``)."""
    engine, ids, query = _contig_and_query(read_placement, reads_kmer_clouds, min_cloud_kmer_freq, reads)
    pos, s0, s1 = engine.score_reads(query, min_position, max_position, min_unit, min_inters)
    return {ids[r]: ((a, b), p if p >= 0 else None) for r, p, a, b in zip(query.tolist(), pos.tolist(), s0.tolist(), s1.tolist())}


def kept_by_map_reads(pos, s0, s1, threshold):
    """map_reads' keep rule (cloud_contig.py:107) on arrays: best_pos == 0, or the score beats the threshold as a tuple, strictly."""
    pos, s0, s1 = np.asarray(pos), np.asarray(s0), np.asarray(s1)
    return (pos == 0) | (s0 > threshold[0]) | ((s0 == threshold[0]) & (s1 > threshold[1]))


def map_reads(read_placement, reads_kmer_clouds, min_cloud_kmer_freq=2, threshold=(5, 10), reads=None):
    """({r_id: position}, {r_id: (s0, s1)}) of the reference's exact ``map_reads`` (cloud_contig.py:98-114): the best start in
    [0, max_pos - units + 1] under calc_inters_score's own thresholds (2, 10) — ``threshold`` plays no part there — kept when it
    is 0 or when its score beats ``threshold``."""
    engine, ids, query = _contig_and_query(read_placement, reads_kmer_clouds, min_cloud_kmer_freq, reads)
    pos, s0, s1 = engine.score_reads(query, None, None, 2, 10)
    keep = kept_by_map_reads(pos, s0, s1, threshold)
    positions, scores = {}, {}
    for r, p, a, b in zip(query[keep].tolist(), pos[keep].tolist(), s0[keep].tolist(), s1[keep].tolist()):
        positions[ids[r]] = p if p >= 0 else None
        scores[ids[r]] = (a, b)
    return positions, scores


class ReadMapper:
    def __init__(self, params):
        from .eltr_polisher import read_reported_positions
        self.params = params
        self.ncrf_report = NCRF_Report(params.ncrf, keep_rows=getattr(params, "n_motif", 1) != 1)
        self.genomic_kmers = _host.read_kmers(params.genomic_kmers, params.k_cloud)
        if self.genomic_kmers.size > 1 and not (self.genomic_kmers[1:] > self.genomic_kmers[:-1]).all():
            self.genomic_kmers = np.unique(self.genomic_kmers)
        extra = km.exotic_lines(params.genomic_kmers, params.k_cloud)      # k-mers with an N (...): no 2-bit code, kept as strings
        if extra:
            self.genomic_kmers = km.KmerSet(self.genomic_kmers, params.k_cloud, extra)
        self.read_placement = read_reported_positions(params.read_placement)
        os.makedirs(params.outdir, exist_ok=True)
        self.outfile = os.path.join(params.outdir, "mapped_positions.csv")

    def clouds(self):
        """The clouds the placer worked on (read_placer.py:103-108): the genomic k-mers, multiplicity filter applied."""
        p = self.params
        clouds = get_reads_kmer_clouds(self.ncrf_report, n=p.n_motif, k=p.k_cloud, genomic_kmers=self.genomic_kmers)
        return filter_reads_kmer_clouds(clouds, min_mult=p.min_kmer_mult)

    def run(self):
        p = self.params
        ids = self.ncrf_report.packed.ids
        known = set(ids)
        unknown = [r_id for r_id in self.read_placement if r_id not in known]
        if unknown:
            raise ValueError(f"{p.read_placement} names reads that are not in the report: {unknown[:3]}")
        if getattr(p, "only_unplaced", False):
            query = [r_id for r_id in ids if self.read_placement.get(r_id) is None]
        else:
            query = list(ids)
        clouds = self.clouds()
        threshold = (p.min_unit, p.min_inters)
        check = getattr(p, "check_exact", False)
        fast = map_reads_fast(self.read_placement, clouds, p.min_cloud_kmer_freq, threshold, reads=query, debug=check)
        positions, scores = fast[0], fast[1]
        self._write("mapped_positions.csv", self._position_lines(query, positions, scores))
        if check:
            self._write("mapping_disagreements.csv", [f"{r_id} {fp} {fs[0]} {fs[1]} {xp} {xs[0]} {xs[1]}" for r_id, fs, xs, fp, xp in fast[2]])
        if getattr(p, "exact", False):
            xpos, xscores = map_reads(self.read_placement, clouds, p.min_cloud_kmer_freq, threshold, reads=query)
            self._write("mapped_positions_exact.csv", self._position_lines(query, xpos, xscores))
        if getattr(p, "rescore_placed", False):
            placed = [r_id for r_id in ids if self.read_placement.get(r_id) is not None]
            at = [self.read_placement[r_id] for r_id in placed]
            got = calc_inters_score(self.read_placement, clouds, p.min_cloud_kmer_freq, reads=placed, min_position=at, max_position=at,
                                    min_unit=0, min_inters=0) if placed else {}
            self._write("placement_scores.csv", [f"{r_id} {got[r_id][1]} {got[r_id][0][0]} {got[r_id][0][1]}" for r_id in placed])
        return positions, scores

    @staticmethod
    def _position_lines(query, positions, scores):
        return [f"{r_id} {positions[r_id]} {scores[r_id][0]} {scores[r_id][1]}" if r_id in positions else f"{r_id} None" for r_id in query]

    def _write(self, name, lines):
        path = os.path.join(self.params.outdir, name)
        with open(path + ".tmp", "w") as f:
            f.writelines(ln + "\n" for ln in lines)
        os.replace(path + ".tmp", path)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Map reads onto the contig of the placed reads of a read_positions.csv")
    p.add_argument("--ncrf", required=True, help="NCRF report on reads")
    p.add_argument("--genomic-kmers", required=True, help="Unique genomic kmers")
    p.add_argument("--read-placement", required=True, help="read_positions.csv of read_placer.py: its placed reads are the contig")
    p.add_argument("--n-motif", type=int, default=1, help="Number of motifs stuck together")
    p.add_argument("--k-cloud", type=int, default=19, help="Size of k-mer for k-mer cloud")
    p.add_argument("--min-cloud-kmer-freq", type=int, default=2, help="Minimal frequency of a kmer in the cloud")
    p.add_argument("--min-kmer-mult", type=int, default=2, help="Minimal frequency of a kmer in input")
    p.add_argument("--min-unit", type=int, default=5, help="threshold[0]: units of the read with a hit")
    p.add_argument("--min-inters", type=int, default=10, help="threshold[1]: hits")
    p.add_argument("--only-unplaced", action="store_true", help="map only the reads without a position in --read-placement")
    p.add_argument("--exact", action="store_true",
                   help="also write mapped_positions_exact.csv: the reference's exact map_reads with threshold (--min-unit, --min-inters)")
    p.add_argument("--check-exact", action="store_true",
                   help="also write mapping_disagreements.csv: the mapped reads whose exact answer differs (map_reads_fast(debug=True))")
    p.add_argument("--rescore-placed", action="store_true",
                   help="also write placement_scores.csv: the exact score of every placed read of --read-placement at its own position")
    p.add_argument("--outdir", required=True, help="Output directory")
    return p.parse_args(argv)


def main(argv=None):
    ReadMapper(parse_args(argv)).run()


if __name__ == "__main__":
    main()

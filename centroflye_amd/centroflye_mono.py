"""The cen6 pipeline's driver up to the polished scaffolds: the drop-in for the reference's ``scripts/centroFlyeMono.py`` as far as this
project builds it.  It takes the reference's arguments and ``--stop-after {correction,graph,mapping,scaffolds,pseudounits,polishing}``;
without ``--stop-after`` it refuses at once and writes nothing: what follows polishing in the reference, its hand-made join of the
first two scaffolds, is not built.

With it: the report is read (``SD_Report``), the monostrings are corrected (``error_correction``, verbose, on a copy), the iterative
de Bruijn graph is built for k = --min-k .. --max-k, the corrected reads are mapped to the graph of --max-k (``map_reads``, one
device call), the long edges are chained into scaffolds (``scaffolding``), the reads are laid on the scaffolds (``read2scaffolds``,
``cover_scaffolds_w_reads``) and the pseudounits with the reads that cover them are cut out (``extract_read_pseudounits``); the
reference's progress lines are printed.  The reference joins its first two scaffolds by hand for cen6 and fails with fewer than two;
here every scaffold goes to the three later calls as the list they take, and no scaffold gives empty files.  Files of our own are
written, each through ``.tmp`` and a rename (formats: INTEGRATION.md):
  OUTDIR/ec_monostrings.tsv    id, part ('.' for an uncut read), strand, string — one line per corrected read, in output order
  OUTDIR/idb/contigs.tsv       k, contig — the contigs of every k, sorted
  OUTDIR/idb/edges.tsv         the graph of --max-k: index in edges() order, u, v, key, colour, length, median coverage, sequence
  OUTDIR/mappings.tsv          id, part, first hit, last hit (edge:letter:read position), valid, path as edge indices; '.' without a hit
  OUTDIR/scaffolds.tsv         index, edge indices, sequence
  OUTDIR/pseudounits.tsv       scaffold, unit, st, en, number of reads
  OUTDIR/read_pseudounits.tsv  scaffold, unit, id, part, st, en, strand — sorted by id and part within a unit
``--stop-after polishing`` then reads --centromeric-reads (FASTA or FASTQ, plain or gzip) and hands every scaffold to ``polish``
(debruijn_graph.py), which writes OUTDIR/polishing: with ``--polisher flye`` (the default, as the reference) one Flye run per
pseudounit, with ``--polisher consensus`` the built-in polisher and no external program.  A refusal of ``polish`` exits non-zero and
leaves no polishing directory."""
import argparse
import os
import sys

import numpy as np

from .debruijn_graph import PolishError, cover_scaffolds_w_reads, extract_read_pseudounits, iterative_graph, polish, read2scaffolds, scaffolding
from .mono_error_correction import error_correction
from .read_recruitment import iter_seqs
from .sd_parser import SD_Report

STAGES = ('correction', 'graph', 'mapping', 'scaffolds', 'pseudounits', 'polishing')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="The cen6 pipeline from the String Decomposer report to the polished scaffolds")
    parser.add_argument('--sd-report', help='the String Decomposer report (decomposition.tsv)', required=True)
    parser.add_argument('--monomers', help='FASTA of the monomers the report was made with', required=True)
    parser.add_argument('--centromeric-reads', help='the centromeric reads, FASTA or FASTQ, plain or gzip (read by the polishing stage only)', required=True)
    parser.add_argument('--outdir', help='directory the files are written to', required=True)
    parser.add_argument('--min-k', help='smallest k of the iterative graph', type=int, default=100)
    parser.add_argument('--max-k', help='largest k of the iterative graph', type=int, default=400)
    parser.add_argument('--min-mult', help='windows a mono-k-mer needs to count as frequent', type=int, default=5)
    parser.add_argument('--polish-n-iter', help='polishing rounds (polishing stage only)', type=int, default=2)
    parser.add_argument('--polish-n-threads', help='threads of a Flye run (polishing stage with --polisher flye only)', type=int, default=50)
    parser.add_argument('--polisher', choices=('flye', 'consensus'), default='flye',
                        help="flye: one external Flye run per pseudounit, as the reference; consensus: the built-in polisher, no external program")
    parser.add_argument('--flye-bin', help='the Flye binary (--polisher flye)', default='flye')
    parser.add_argument('--consensus-max-divergence-permille', type=int, default=300,
                        help='--polisher consensus: a read votes if its edit distance to the template is at most this many thousandths of the template length')
    parser.add_argument('--uncovered-pseudounits', choices=('refuse', 'monomers'), default='refuse',
                        help="a pseudounit no read covers: refuse, or take the concatenation of its letters' monomers, unpolished")
    parser.add_argument('--stop-after', choices=STAGES, help="Stop after this stage (required: the reference's manual join of scaffolds behind polishing is not built)")
    params = parser.parse_args(argv)
    if params.consensus_max_divergence_permille < 0:
        parser.error('--consensus-max-divergence-permille must not be negative')
    return params


def _write(path, lines):
    tmp = path + '.tmp'
    with open(tmp, 'w') as f:
        f.writelines(lines)
    os.replace(tmp, path)


def _id_part(key):
    return (key[0], str(key[1])) if isinstance(key, tuple) else (key, '.')


def ec_lines(ec_monostrings):
    for key, ms in ec_monostrings.items():
        r_id, part = _id_part(key)
        yield f'{r_id}\t{part}\t{ms.strand}\t{ms.tostring()}\n'


def contig_lines(contigs):
    for k in sorted(contigs):
        for contig in sorted(contigs[k]):
            yield f'{k}\t{contig}\n'


def edge_lines(edges):
    """edges: [(u, v, key, colour, coverages, sequence)] in edges() order"""
    for x, (u, v, key, colour, coverages, seq) in enumerate(edges):
        yield f'{x}\t{u}\t{v}\t{key}\t{colour}\t{len(coverages)}\t{float(np.median(coverages)):g}\t{seq}\n'


def mapping_lines(mappings, edge_index):
    for key, m in mappings.items():
        r_id, part = _id_part(key)
        if m is None:
            yield f'{r_id}\t{part}\t.\t.\t.\t.\n'
            continue
        ((e0, j0), i0), ((e1, j1), i1), valid, path = m
        yield f'{r_id}\t{part}\t{e0}:{j0}:{i0}\t{e1}:{j1}:{i1}\t{int(bool(valid))}\t{",".join(str(edge_index[tuple(e)]) for e in path)}\n'


def scaffold_lines(scaffolds, edge_scaffolds, edge_index):
    for x, (seq, path) in enumerate(zip(scaffolds, edge_scaffolds)):
        yield f'{x}\t{",".join(str(edge_index[tuple(e)]) for e in path)}\t{seq}\n'


def pseudounit_lines(pseudounits, read_pseudounits):
    for s, (units, reads) in enumerate(zip(pseudounits, read_pseudounits)):
        for x, ((st, en), covering) in enumerate(zip(units, reads)):
            yield f'{s}\t{x}\t{st}\t{en}\t{len(covering)}\n'


def read_pseudounit_lines(read_pseudounits):
    for s, reads in enumerate(read_pseudounits):
        for x, covering in enumerate(reads):
            for r_id, part, st, en, strand in sorted(_id_part(key) + tuple(v) for key, v in covering.items()):
                yield f'{s}\t{x}\t{r_id}\t{part}\t{st}\t{en}\t{strand}\n'


def main(argv=None):
    params = parse_args(argv)
    if params.stop_after is None:
        sys.exit("centroFlyeMono: the reference's hand-made join of scaffolds that follows polishing is not built; run with --stop-after " + ', '.join(STAGES[:-1]) +
                 ' or ' + STAGES[-1])
    stop = STAGES.index(params.stop_after)
    os.makedirs(params.outdir, exist_ok=True)

    print('Reading report')
    sd_report = SD_Report(SD_report_fn=params.sd_report, monomers_fn=params.monomers)

    print('Error correcting monoreads')
    ec_monostrings = error_correction(sd_report.monostrings, verbose=True, inplace=False)
    _write(os.path.join(params.outdir, 'ec_monostrings.tsv'), ec_lines(ec_monostrings))
    if stop == 0:
        return 0

    print('Building the graph')
    idb = os.path.join(params.outdir, 'idb')
    contigs, dbs, _, _ = iterative_graph(ec_monostrings, min_k=params.min_k, max_k=params.max_k, outdir=idb, min_mult=params.min_mult)
    _write(os.path.join(idb, 'contigs.tsv'), contig_lines(contigs))
    if stop == 1:
        return 0

    print('Mapping reads to the graph')
    db = dbs[params.max_k]
    db_edges = db.graph.edges()
    edge_index = {e: x for x, e in enumerate(db_edges)}
    datas = [db.graph.data(*e) for e in db_edges]
    _write(os.path.join(idb, 'edges.tsv'), edge_lines([e + (d['color'], d['coverages'], d['edge_kmer']) for e, d in zip(db_edges, datas)]))
    mappings = db.map_reads(ec_monostrings, verbose=False)
    _write(os.path.join(params.outdir, 'mappings.tsv'), mapping_lines(mappings, edge_index))
    if stop == 2:
        return 0

    print('Scaffolding')
    scaffolds, edge_scaffolds = scaffolding(db, mappings)
    _write(os.path.join(params.outdir, 'scaffolds.tsv'), scaffold_lines(scaffolds, edge_scaffolds, edge_index))
    if stop == 3:
        return 0

    print('Mapping reads to scaffolds')
    r2s = read2scaffolds(db, edge_scaffolds, mappings, ec_monostrings)
    print('Covering scaffolds with reads')
    coverage = cover_scaffolds_w_reads(r2s, mappings, scaffolds, ec_monostrings, k=db.k)
    print('Extracting pseudounits and reads covering them')
    pseudounits, read_pseudounits = extract_read_pseudounits(coverage, scaffolds, monostrings=ec_monostrings)
    _write(os.path.join(params.outdir, 'pseudounits.tsv'), pseudounit_lines(pseudounits, read_pseudounits))
    _write(os.path.join(params.outdir, 'read_pseudounits.tsv'), read_pseudounit_lines(read_pseudounits))
    if stop == 4:
        return 0

    print('Reading centromeric reads')
    centromeric_reads = {name.decode(): seq.decode('latin-1') for name, seq in iter_seqs(params.centromeric_reads)}
    monomers = {name.decode(): seq.decode('latin-1') for name, seq in iter_seqs(params.monomers)}
    print('Polishing')
    try:
        polish(scaffolds=scaffolds, pseudounits=pseudounits, read_pseudounits=read_pseudounits, reads=centromeric_reads, monomers=monomers,
               outdir=os.path.join(params.outdir, 'polishing'), n_iter=params.polish_n_iter, n_threads=params.polish_n_threads, flye_bin=params.flye_bin,
               polisher=params.polisher, permille=params.consensus_max_divergence_permille, uncovered=params.uncovered_pseudounits)
    except PolishError as e:
        sys.exit(f'centroFlyeMono: {e}')
    return 0

"""The cen6 pipeline's driver up to the graph: the drop-in for the reference's ``scripts/centroFlyeMono.py`` as far as this project
builds it.  It takes the reference's arguments and ``--stop-after {correction,graph}``; without ``--stop-after`` it refuses at once
(mapping reads to the graph, scaffolding, pseudounits and polishing are not built) and writes nothing.

With it: the report is read (``SD_Report``), the monostrings are corrected (``error_correction``, verbose, on a copy) and, for
``graph``, the iterative de Bruijn graph is built for k = --min-k .. --max-k; the reference's progress lines are printed.  Two files
of our own are written, each through ``.tmp`` and a rename (formats: INTEGRATION.md):
  OUTDIR/ec_monostrings.tsv   id, part ('.' for an uncut read), strand, string — one line per corrected read, in output order
  OUTDIR/idb/contigs.tsv      k, contig — the contigs of every k, sorted"""
import argparse
import os
import sys

from .debruijn_graph import iterative_graph
from .mono_error_correction import error_correction
from .sd_parser import SD_Report


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Monostring error correction and the iterative de Bruijn graph of the cen6 pipeline")
    parser.add_argument('--sd-report', help='the String Decomposer report (decomposition.tsv)', required=True)
    parser.add_argument('--monomers', help='FASTA of the monomers the report was made with', required=True)
    parser.add_argument('--centromeric-reads', help='the centromeric reads (read by the polishing stage only: accepted, unused)', required=True)
    parser.add_argument('--outdir', help='directory the two files are written to', required=True)
    parser.add_argument('--min-k', help='smallest k of the iterative graph', type=int, default=100)
    parser.add_argument('--max-k', help='largest k of the iterative graph', type=int, default=400)
    parser.add_argument('--min-mult', help='windows a mono-k-mer needs to count as frequent', type=int, default=5)
    parser.add_argument('--polish-n-iter', help='polishing rounds (accepted, unused)', type=int, default=2)
    parser.add_argument('--polish-n-threads', help='polishing threads (accepted, unused)', type=int, default=50)
    parser.add_argument('--stop-after', choices=('correction', 'graph'),
                        help='Stop after this stage (required: the stages behind the graph are not built)')
    return parser.parse_args(argv)


def _write(path, lines):
    tmp = path + '.tmp'
    with open(tmp, 'w') as f:
        f.writelines(lines)
    os.replace(tmp, path)


def ec_lines(ec_monostrings):
    for key, ms in ec_monostrings.items():
        r_id, part = (key[0], str(key[1])) if isinstance(key, tuple) else (key, '.')
        yield f'{r_id}\t{part}\t{ms.strand}\t{ms.tostring()}\n'


def contig_lines(contigs):
    for k in sorted(contigs):
        for contig in sorted(contigs[k]):
            yield f'{k}\t{contig}\n'


def main(argv=None):
    params = parse_args(argv)
    if params.stop_after is None:
        sys.exit('centroFlyeMono: mapping reads to the graph, scaffolding, pseudounits and polishing are not built; '
                 'run with --stop-after correction or --stop-after graph')
    os.makedirs(params.outdir, exist_ok=True)

    print('Reading report')
    sd_report = SD_Report(SD_report_fn=params.sd_report, monomers_fn=params.monomers)

    print('Error correcting monoreads')
    ec_monostrings = error_correction(sd_report.monostrings, verbose=True, inplace=False)
    _write(os.path.join(params.outdir, 'ec_monostrings.tsv'), ec_lines(ec_monostrings))
    if params.stop_after == 'correction':
        return 0

    print('Building the graph')
    idb = os.path.join(params.outdir, 'idb')
    contigs, _, _, _ = iterative_graph(ec_monostrings, min_k=params.min_k, max_k=params.max_k, outdir=idb, min_mult=params.min_mult)
    _write(os.path.join(idb, 'contigs.tsv'), contig_lines(contigs))
    return 0

"""The polisher stage: per-position read-unit export, one Flye run per position, and the assembly
of the polished units into the final sequence of every iteration with its report.

Mirror of the reference's ``scripts/eltr_polisher.py``.  The pure data movement — ``read_reported_positions`` (:19-30),
``ELTR_Polisher.__init__`` (:33-51, the ``max_pos`` default), ``map_pos2read`` (:53-66) and ``export_read_units`` (:68-97) —
groups and writes in the compiled host library (``cfh_export_read_units``: one pass over the packed units, positions written
by a thread pool).  ``run_polishing`` (:99-114) starts the same Flye command per position.  ``read_polishing`` (:116-131),
``compare_polished_sequences`` (:133-146) and ``export_results`` (:148-157) are ``assemble``: the final sequences go to the
device once, one ``cf_hpc`` call compresses them all and one ``cf_edit_distances`` call gives every distance of ``report.txt``
(DESIGN §16).

``--polisher consensus`` takes Flye's place with the library's own polisher (``cf_consensus_run``): every position's
template and reads, as the export wrote them, go to the device in one call, and the ``pos_P/polished_i.fasta`` it writes are
what ``assemble`` consumes.  It is not Flye's polisher and does not reproduce Flye's output; ``--polisher flye`` stays the default.

Without ``--num-iters``, ``--polish``, ``--assemble-only`` or ``--polisher consensus`` the script ends with the exported files, as
it always did.
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np

from . import ncrf_parser

DEFAULT_MAX_DIVERGENCE_PERMILLE = 300  # --consensus-max-divergence-permille: a read votes iff 1000 d <= permille x template length
DEFAULT_MAX_EDIT_DISTANCE = 32768      # --max-edit-distance (65 536 took 2.5 s to give up on two unrelated 1-Mb strings, this 0.64 s)


class PolishingError(RuntimeError):
    """What makes the reference raise in read_polishing: a polished_i.fasta that is missing or empty, a position without reads."""


def read_first_record(fn):
    """The sequence of the first record of a FASTA file (the reference's read_bio_seq, utils/bio.py:11-13): lines joined."""
    try:
        f = open(fn)
    except OSError as e:
        raise PolishingError(f"{fn}: {e.strerror or e}") from None
    with f:
        lines, inside = [], False
        for ln in f:
            if ln[:1] == ">":
                if inside:
                    break
                inside = True
            elif inside:
                lines.append(ln.strip())
    if not inside:
        raise PolishingError(f"{fn}: no FASTA record")
    return "".join(lines).replace(" ", "")


def read_records(fn):
    """The sequences of all records of a FASTA file, in file order (lines joined, like read_first_record)."""
    try:
        f = open(fn)
    except OSError as e:
        raise PolishingError(f"{fn}: {e.strerror or e}") from None
    seqs = []
    with f:
        for ln in f:
            if ln[:1] == ">":
                seqs.append([])
            elif seqs:
                seqs[-1].append(ln.strip())
    return ["".join(x).replace(" ", "") for x in seqs]


def alignment_dict(distance, query, target):
    """What python-edlib 1.2.4 returns for edlib.align(query, target) (mode NW, task distance) and the reference prints."""
    if distance < 0:
        return {'editDistance': -1, 'alphabetLength': len(set(query) | set(target)), 'locations': None, 'cigar': None}
    return {'editDistance': int(distance), 'alphabetLength': len(set(query) | set(target)), 'locations': [(None, len(target) - 1)],
            'cigar': None}


def _write_atomically(files):
    """{path: text}: every file through path.tmp, renamed only when all are written."""
    tmp = []
    try:
        for fn, text in files.items():
            with open(fn + ".tmp", "w") as f:
                f.write(text)
            tmp.append(fn)
    except BaseException:
        for fn in tmp + [fn]:
            if os.path.exists(fn + ".tmp"):
                os.remove(fn + ".tmp")
        raise
    for fn in tmp:
        os.replace(fn + ".tmp", fn)


def read_reported_positions(read_positions_fn):
    """{r_id: position or None} in file order (reference :19-30: split on ' ', field 1, 'None' -> None)."""
    pos = {}
    with open(read_positions_fn) as f:
        for line in f:
            fields = line.strip().split(' ')
            pos[fields[0]] = None if fields[1] == 'None' else int(fields[1])
    return pos


class ELTR_Polisher:
    def __init__(self, params):
        self.params = params
        if not os.path.isfile(params.unit):
            raise FileNotFoundError(f"File {params.unit} is not found")
        self.ncrf_report = ncrf_parser.NCRF_Report(params.ncrf)
        os.makedirs(params.outdir, exist_ok=True)
        self.read_placement = read_reported_positions(params.read_placement)
        self.min_pos = params.min_pos
        self.max_pos = params.max_pos
        packed = self.ncrf_report.packed
        self._index = {r_id: i for i, r_id in enumerate(packed.ids)}
        self._n_units = (packed.units(1)[0][1:] - packed.units(1)[0][:-1])
        if self.max_pos == math.inf:
            self.max_pos = 0
            for r_id, pos in self.read_placement.items():
                if pos is not None:
                    self.max_pos = max(self.max_pos, pos + int(self._n_units[self._index[r_id]]))

    def map_pos2read(self):
        """{position: [(r_id, unit index), ...]} — small-object form of what the exporter groups natively."""
        pos2read = {}
        for r_id, pos in self.read_placement.items():
            if pos is None or pos > self.max_pos:
                continue
            n = int(self._n_units[self._index[r_id]])
            units = range(n) if (pos == self.min_pos or pos + n == self.max_pos) else range(1, n - 1)
            for i in units:
                if self.min_pos <= pos + i <= self.max_pos:
                    pos2read.setdefault(pos + i, []).append((r_id, i))
        return pos2read

    def export_read_units(self, pos2read=None):
        """Writes pos_P/read_units.fasta and pos_P/median_read_unit.fasta for every position; returns
        {position: (units_fn, median_read_unit_fn)} like the reference.  ``pos2read`` is accepted for signature
        parity; the files are produced from the placement itself by the native exporter."""
        placed = [(self._index[r_id], pos) for r_id, pos in self.read_placement.items() if pos is not None]
        rec = [x[0] for x in placed]
        pos = [x[1] for x in placed]
        self.ncrf_report.packed.export_read_units(rec, pos, self.params.outdir, self.min_pos, self.max_pos)
        positions = pos2read.keys() if pos2read is not None else self.map_pos2read().keys()
        return {p: (os.path.join(self.params.outdir, f'pos_{p}', 'read_units.fasta'),
                    os.path.join(self.params.outdir, f'pos_{p}', 'median_read_unit.fasta')) for p in positions}

    def unit_filenames(self, pos2read):
        """{position: (units_fn, median_read_unit_fn)} as export_read_units returns it, without exporting (--assemble-only)."""
        return {p: (os.path.join(self.params.outdir, f'pos_{p}', 'read_units.fasta'),
                    os.path.join(self.params.outdir, f'pos_{p}', 'median_read_unit.fasta')) for p in pos2read}

    def run_polishing(self, read_unit_filenames):
        """One Flye process per position (reference :99-114, the same argument vector)."""
        p = self.params
        for pos in range(min(read_unit_filenames), max(read_unit_filenames) + 1):
            if pos not in read_unit_filenames:
                raise PolishingError(f"position {pos} has no reads")
            units_fn, median_read_unit_fn = read_unit_filenames[pos]
            cmd = [getattr(p, "flye_bin", "flye"), f'--{getattr(p, "error_mode", "nano")}-raw', units_fn, '--polish-target', median_read_unit_fn,
                   '-i', getattr(p, "num_iters", None) or 4, '-t', getattr(p, "num_threads", 16), '-o', os.path.dirname(units_fn)]
            cmd = [str(x) for x in cmd]
            print(' '.join(cmd))
            subprocess.check_call(cmd)

    def run_consensus(self, read_unit_filenames, num_iters=None, permille=None):
        """The built-in polisher in Flye's place: the first record of median_read_unit.fasta and the records of read_units.fasta of
        every position, in file order, one cf_consensus_run, then pos_P/polished_i.fasta (header >consensus_pos_P_iter_i) and
        consensus_report.tsv.  Nothing is written when a position of min .. max has no reads or a string is beyond the device's
        limit."""
        from . import session
        p = self.params
        num_iters = int(num_iters if num_iters is not None else (getattr(p, "num_iters", None) or 4))
        permille = int(permille if permille is not None else getattr(p, "consensus_max_divergence_permille", DEFAULT_MAX_DIVERGENCE_PERMILLE))
        if num_iters < 1:
            raise PolishingError("--num-iters must be at least 1")
        if not read_unit_filenames:
            raise PolishingError("no position has reads")
        positions = list(range(min(read_unit_filenames), max(read_unit_filenames) + 1))
        for pos in positions:
            if pos not in read_unit_filenames:
                raise PolishingError(f"position {pos} has no reads")
        e = session.engine()
        max_len = e.consensus_info()["max_len"]
        templates, reads = [], []
        for pos in positions:
            units_fn, median_read_unit_fn = read_unit_filenames[pos]
            templates.append(read_first_record(median_read_unit_fn).encode("latin-1"))
            reads.append([r.encode("latin-1") for r in read_records(units_fn)])
            if not reads[-1]:
                raise PolishingError(f"position {pos} has no reads")
            longest = max(len(templates[-1]), max(len(r) for r in reads[-1]))
            if longest > max_len:
                raise PolishingError(f"position {pos} has a sequence of {longest} bases, more than the {max_len} --polisher consensus takes")
        t_off = np.zeros(len(positions) + 1, np.int64)
        np.cumsum([len(t) for t in templates], out=t_off[1:])
        pos_ptr = np.zeros(len(positions) + 1, np.int64)
        np.cumsum([len(rs) for rs in reads], out=pos_ptr[1:])
        flat = [r for rs in reads for r in rs]
        r_off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(r) for r in flat], out=r_off[1:])
        res = e.consensus_run(b"".join(templates), t_off, b"".join(flat), r_off, pos_ptr, num_iters, permille)
        self.consensus_ms = e.consensus_info()["phase_ms"]
        files, rows = {}, ["iteration\tposition\ttemplate_length\treads\tvoting\texcluded\toutput_length"]
        lengths = np.diff(t_off)
        for i, (b, off, n_voting, n_excluded) in enumerate(res, 1):
            text = b.tobytes().decode("latin-1")
            for j, pos in enumerate(positions):
                files[os.path.join(os.path.dirname(read_unit_filenames[pos][0]), f'polished_{i}.fasta')] = \
                    f'>consensus_pos_{pos}_iter_{i}\n{text[off[j]:off[j + 1]]}\n'
                rows.append(f"{i}\t{pos}\t{int(lengths[j])}\t{len(reads[j])}\t{int(n_voting[j])}\t{int(n_excluded[j])}\t{int(off[j + 1] - off[j])}")
            lengths = np.diff(off)
        files[os.path.join(p.outdir, 'consensus_report.tsv')] = "".join(r + "\n" for r in rows)
        _write_atomically(files)

    def read_polishing(self, read_unit_filenames, num_iters):
        """{position: [polished sequence of iteration 1 .. num_iters]} (reference :116-126) after the checks that make the
        reference raise: every position of min .. max has reads, every polished_i.fasta is there."""
        if not read_unit_filenames:
            raise PolishingError("no position has reads")
        for pos in range(min(read_unit_filenames), max(read_unit_filenames) + 1):
            if pos not in read_unit_filenames:
                raise PolishingError(f"position {pos} has no reads")
        return {pos: [read_first_record(os.path.join(os.path.dirname(fns[0]), f'polished_{i}.fasta')) for i in range(1, num_iters + 1)]
                for pos, fns in sorted(read_unit_filenames.items())}

    def assemble(self, read_unit_filenames, num_iters=None, max_edit_distance=None, position_report=None):
        """final_sequence_i.fasta, final_sequence_hpc_i.fasta and report.txt (reference :116-157) — and position_changes.csv —
        from the polished_i.fasta of every position.  Returns the distances [(plain, compressed) for i = 1 .. num_iters - 1],
        -1 standing for "above the limit"."""
        from . import session
        p = self.params
        num_iters = int(num_iters if num_iters is not None else (getattr(p, "num_iters", None) or 4))
        limit = int(max_edit_distance if max_edit_distance is not None else getattr(p, "max_edit_distance", DEFAULT_MAX_EDIT_DISTANCE))
        position_report = getattr(p, "position_report", False) if position_report is None else position_report
        if num_iters < 1:
            raise PolishingError("--num-iters must be at least 1")
        polished = self.read_polishing(read_unit_filenames, num_iters)
        positions = sorted(polished)
        finals = ["".join(polished[pos][i] for pos in positions).encode("latin-1") for i in range(num_iters)]
        e = session.engine()
        off = np.zeros(num_iters + 1, np.int64)
        np.cumsum([len(s) for s in finals], out=off[1:])
        hpc, hpc_off = e.hpc(b"".join(finals), off)
        hpc = hpc.tobytes()
        finals_hpc = [hpc[hpc_off[i]:hpc_off[i + 1]] for i in range(num_iters)]
        dists = []
        if num_iters > 1:
            # the strings of either side of a pair list lie back to back, so ONE call takes the pairs (i, i + 1) of the plain
            # sequences, two pairs that join the runs — (the last plain sequence, nothing) and (nothing, the first compressed
            # one): an empty string costs no step — and the pairs of the compressed sequences, all on the bytes cf_hpc left
            # on the device: its input followed by its output
            h = off[-1] + hpc_off
            a_off = np.concatenate([off, off[-1:], h[1:num_iters]])
            b_off = np.concatenate([off[1:], off[-1:], h[1:]])
            d, self.edit_ms = e.edit_distances(None, a_off, b_off, limit)
            dists = [(int(d[i]), int(d[num_iters + 1 + i])) for i in range(num_iters - 1)]
        files = {}
        lines = []
        for i in range(1, num_iters):
            for what, seqs, dist in (("polishing", finals, dists[i - 1][0]), ("homopolymer compressed polishing", finals_hpc, dists[i - 1][1])):
                lines.append(f'Alignment {what} seq {i} vs {i+1}:')
                lines.append(str(alignment_dict(dist, seqs[i - 1], seqs[i])))
                if dist < 0:
                    print(f"eltr_polisher: the {what} sequences {i} and {i+1} differ in more than {limit} places (--max-edit-distance): "
                          "reported as -1", file=sys.stderr)
        files[os.path.join(p.outdir, 'report.txt')] = "".join(ln + "\n" for ln in lines)
        for i in range(1, num_iters + 1):
            files[os.path.join(p.outdir, f'final_sequence_{i}.fasta')] = f'>polished_repeat_{i}\n{finals[i - 1].decode("latin-1")}\n'
            files[os.path.join(p.outdir, f'final_sequence_hpc_{i}.fasta')] = f'>polished_repeat_{i}\n{finals_hpc[i - 1].decode("latin-1")}\n'
        if position_report:
            files[os.path.join(p.outdir, 'position_changes.csv')] = self.position_changes(polished, num_iters, limit)
        _write_atomically(files)
        return dists

    def position_changes(self, polished, num_iters, limit):
        """Lines `iteration position distance`: the distance between polished_i and polished_{i+1} of every position, all
        pairs in one cf_edit_distances call."""
        from . import session
        positions = sorted(polished)
        if num_iters < 2 or not positions:
            return ""
        # iteration-major: the strings of iteration i + 1 follow those of iteration i, so a_off = off[:-n], b_off = off[n:]
        seqs = [polished[pos][i].encode("latin-1") for i in range(num_iters) for pos in positions]
        n = len(positions)
        off = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        d, _ = session.engine().edit_distances(b"".join(seqs), off[:len(off) - n], off[n:], limit)
        return "".join(f"{i + 1} {pos} {int(d[i * n + j])}\n" for i in range(num_iters - 1) for j, pos in enumerate(positions))

    def run(self, export_only=True):
        """export_only (the default, and all that a params object without the new attributes asks for): the export alone.
        Otherwise the reference's run(): export, Flye per position, assemble."""
        pos2read = self.map_pos2read()
        if getattr(self.params, "assemble_only", False):
            return self.assemble(self.unit_filenames(pos2read))
        consensus = not export_only and getattr(self.params, "polisher", "flye") == "consensus"
        if consensus:      # known before anything is written
            for pos in range(min(pos2read, default=0), max(pos2read, default=-1) + 1):
                if pos not in pos2read:
                    raise PolishingError(f"position {pos} has no reads")
        files = self.export_read_units(pos2read)
        if export_only:
            return files
        if not files:
            raise PolishingError("no position has reads")
        if consensus:
            self.run_consensus(files)
        else:
            self.run_polishing(files)
        return self.assemble(files)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--read-placement", required=True)
    parser.add_argument("--unit", required=True)
    parser.add_argument("--outdir", required=True)
    parser.add_argument("--ncrf", required=True)
    parser.add_argument("--min-pos", type=int, default=0)
    parser.add_argument("--max-pos", type=int, default=math.inf)
    parser.add_argument("--flye-bin", default='flye')
    parser.add_argument("--error-mode", default="nano")
    parser.add_argument("--num-iters", default=None, type=int, help="Flye polishing iterations (4 when the full stage runs); giving it selects the full stage")
    parser.add_argument("--num-threads", default=16, type=int)
    parser.add_argument("--export-only", action="store_true", help="stop after the per-position export (the default without --num-iters / --polish / --assemble-only)")
    parser.add_argument("--polish", action="store_true", help="the full stage: export, one Flye run per position, assemble")
    parser.add_argument("--assemble-only", action="store_true", help="skip the export and Flye: assemble the pos_P/polished_i.fasta that are there")
    parser.add_argument("--max-edit-distance", type=int, default=DEFAULT_MAX_EDIT_DISTANCE,
                        help="distances above this are reported as -1 (the work grows with its square)")
    parser.add_argument("--position-report", action="store_true", help="also write position_changes.csv: iteration position distance")
    parser.add_argument("--polisher", choices=("flye", "consensus"), default="flye",
                        help="flye (default): one Flye process per position; consensus: the library's own column-vote polisher, all positions in one "
                             "device call, no external program (--flye-bin, --error-mode and --num-threads are ignored); not Flye's output")
    parser.add_argument("--consensus-max-divergence-permille", type=int, default=DEFAULT_MAX_DIVERGENCE_PERMILLE,
                        help="--polisher consensus: a read votes iff 1000 x its edit distance to the template <= this x the template's length")
    params = parser.parse_args()
    if params.max_edit_distance < 0:
        parser.error("--max-edit-distance must not be negative")
    if params.consensus_max_divergence_permille < 0:
        parser.error("--consensus-max-divergence-permille must not be negative")
    full = (params.polish or params.num_iters is not None or params.assemble_only or params.polisher == "consensus") and not params.export_only
    if params.export_only and (params.polish or params.assemble_only):
        parser.error("--export-only excludes --polish and --assemble-only")
    try:
        ELTR_Polisher(params).run(export_only=not full)
    except PolishingError as e:
        sys.exit(f"eltr_polisher: {e}")
    except subprocess.CalledProcessError as e:
        sys.exit(f"eltr_polisher: {e}")


if __name__ == "__main__":
    main()

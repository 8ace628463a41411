"""Monomer strings ("monostrings") from a String Decomposer report: the drop-in for the reference's ``scripts/sd_parser.py``.

The report has one line per monomer instance in six tab-separated columns (sd_parser.py:174-180): read id, monomer name (with an
apostrophe for the reverse-complemented monomer), first and last read base, a score, and the reliability ('+', anything else is a
gap).  ``SD_Report`` turns every read into a ``MonoString``: one letter per reliable instance (A .. Z by the order of the monomers in
the FASTA file, a .. z for the primed ones; a monomer past the 26th has no letter and a report that names it is refused with a
KeyError, as in the reference), ``?`` for an unreliable instance and ``int(round(gap / mean monomer length))`` more for a jump of
more than ``max_gap`` bases between two instances; the string is then stripped of gap symbols at both ends and, when more than half
of its letters are lower case, reversed and case-swapped (strand '-').

What is reproduced on purpose: the reads come out in sorted order of their ids (the reference groups a data frame, which sorts);
the mean monomer length is taken over ALL monomers of the file; the rounding is Python's round-half-even on the double; the
``gap_symb`` given to ``SD_Report`` is kept on the report but the strings are built with '?' (FromSDRecord does not pass it on).
One documented difference: a report whose read ids are all numeric yields ``int`` keys in the reference (the type inference of its
CSV reader); here ids stay strings.  ``MonoString.split`` belongs to the error-correction follow-up and is not here.  The
reference's ``main`` calls a method that ``SD_Report`` does not have; here it prints the statistics of ``.monostrings``, the lines
of ``get_stats(verbose=True)``.

The writer of such reports in this project is ``scripts/monomer_decomposer.py`` (the built-in decomposer: NOT String Decomposer).
No pandas, no Biopython."""
import argparse
from collections import Counter
from itertools import groupby
from string import ascii_lowercase, ascii_uppercase

import numpy as np

from .read_recruitment import iter_seqs


class MonoString:
    def __init__(self, name, string=(), mono2nucl=None, gap_symb='?', strand='+'):
        self.name = name
        self.string = list(string)
        self.mono2nucl = dict(mono2nucl or {})
        self.gap_symb = gap_symb
        self.strand = strand

    @classmethod
    def FromSDRecord(cls, name, monomers, starts, ends, reliability, max_gap, mean_monomer_len, gap_symb):
        ms = cls(name=name)      # (the reference leaves gap_symb at its default here)
        prev_en = None
        for letter, st, en, rel in zip(monomers, starts, ends, reliability):
            if prev_en is not None and st - prev_en > max_gap:
                ms.add_gap(int(round((st - prev_en) / mean_monomer_len)))
            if rel == '+':
                ms.add_monomer(letter, st, en)
            else:
                ms.add_gap(1)
            prev_en = en
        ms.assert_validity()
        ms.strip()
        ms.check_reverse()
        return ms

    def tostring(self):
        return ''.join(self.string)

    def __len__(self):
        return len(self.string)

    def __getitem__(self, sub):
        if isinstance(sub, slice):
            return ''.join(self.string[sub])
        return self.string[sub]

    def __setitem__(self, sub, value):
        if isinstance(sub, slice) and isinstance(value, str):
            value = list(value)
        self.string[sub] = value

    def assert_validity(self):
        for coord, (c, _, _) in self.mono2nucl.items():
            assert 0 <= coord < len(self.string) and c == self.string[coord], (coord, c)

    def add_monomer(self, monomer, st, en):
        self.mono2nucl[len(self.string)] = (monomer, st, en)
        self.string.append(monomer)

    def add_gap(self, length):
        self.string += [self.gap_symb] * length

    def check_reverse(self):
        letters = [c for c in self.string if c.lower() != c.upper()]
        if letters and 2 * sum(c.islower() for c in letters) > len(letters):
            n = len(self.string)
            self.string = [c.swapcase() for c in reversed(self.string)]
            self.strand = '-'
            self.mono2nucl = {n - coord - 1: (c.swapcase(), en, st) for coord, (c, st, en) in self.mono2nucl.items()}
        self.assert_validity()

    def trim_read(self, left, right):
        self.string = self.string[left:right]
        self.mono2nucl = {k - left: v for k, v in self.mono2nucl.items() if left <= k < right}
        self.assert_validity()

    def strip(self):
        i, j = 0, len(self.string) - 1
        while i < len(self.string) and self.string[i] == self.gap_symb:
            i += 1
        while j >= 0 and self.string[j] == self.gap_symb:
            j -= 1
        self.trim_read(i, j + 1)


def _monomer_lengths(monomers_fn):
    """{name: length} in file order (a repeated name keeps its first place and its last length, as a dict does)"""
    lens = {}
    for name, seq in iter_seqs(monomers_fn):
        lens[name.decode()] = len(seq)
    return lens


class SD_Report:
    def __init__(self, SD_report_fn, monomers_fn, max_gap=100, gap_symb='?'):
        self.gap_symb = gap_symb
        lens = _monomer_lengths(monomers_fn)
        mean_monomer_len = float(np.mean(list(lens.values())))
        self.monomer_names_map = {}
        self.rev_monomer_names_map = {}
        for name, ucode, lcode in zip(lens, ascii_uppercase, ascii_lowercase):
            self.monomer_names_map[name] = ucode
            self.monomer_names_map[name + "'"] = lcode
            self.rev_monomer_names_map[ucode] = name
        rows = {}
        with open(SD_report_fn) as f:
            for line in f:
                line = line.rstrip("\r\n")
                if not line:
                    continue
                r_id, monomer, st, en, _score, rel = line.split("\t")[:6]
                rows.setdefault(r_id, []).append((self.monomer_names_map[monomer], int(st), int(en), rel))
        self.monostrings = {}
        for r_id in sorted(rows):
            letters, starts, ends, rels = zip(*rows[r_id])
            self.monostrings[r_id] = MonoString.FromSDRecord(name=r_id, monomers=list(letters), starts=list(starts), ends=list(ends),
                                                             reliability=list(rels), max_gap=max_gap,
                                                             mean_monomer_len=mean_monomer_len, gap_symb=self.gap_symb)


def get_ngap_symbols(monostrings, compr_hmp=False, gap_symb='?'):
    cnt = 0
    for monostring in monostrings.values():
        symbols = list(monostring)
        if compr_hmp:
            symbols = [x for x, _ in groupby(symbols)]
        cnt += Counter(symbols)[gap_symb]
    return cnt


def get_stats(monostrings, verbose=False, return_stats=True):
    stats = {}
    lens = [len(monostr) for monostr in monostrings.values()]
    stats['ntranslations'] = len(lens)
    stats['min_len'] = np.min(lens)
    stats['max_len'] = np.max(lens)
    stats['mean_len'] = np.mean(lens)
    stats['tot_len'] = np.sum(lens)
    stats['ngaps'] = get_ngap_symbols(monostrings)
    stats['pgaps'] = stats['ngaps'] / stats['tot_len']
    stats['ngap_runs'] = get_ngap_symbols(monostrings, compr_hmp=True)
    if verbose:
        print(f'Number of translations: {stats["ntranslations"]}')
        print(f'Min length = {stats["min_len"]}')
        print(f'Mean length = {stats["mean_len"]}')
        print(f'Max length = {stats["max_len"]}')
        print(f'Total length = {stats["tot_len"]}')
        print(f'#(%) Gap symbols = {stats["ngaps"]} ({stats["pgaps"]})')
        print(f'#Gap runs = {stats["ngap_runs"]}')
    if return_stats:
        return stats


def main(argv=None):
    parser = argparse.ArgumentParser(description="Statistics of the monostrings of a String Decomposer report")
    parser.add_argument("-i", "--input", help="Report of SD", required=True)
    parser.add_argument("-m", "--monomers", help="Fasta with monomers", required=True)
    params = parser.parse_args(argv)
    sd_report = SD_Report(params.input, params.monomers)
    get_stats(monostrings=sd_report.monostrings, verbose=True, return_stats=False)
    return 0

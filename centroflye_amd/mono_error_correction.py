"""Error correction of monostrings: the drop-in for the reference's ``scripts/mono_error_correction.py`` (the second call of
``centroFlyeMono.py``'s main), with its signatures, defaults, return values and ``verbose`` lines.

The steps, as the reference runs them: reads with more than a tenth of lower-case letters are dropped; every read is trimmed to the
stretch between the first and the last window of ``ma_window`` letters whose share of gaps is at most ``max_gap`` and stripped of
gaps at its ends; a read with more than 5 % gaps is cut at its gaps into parts of at least ``min_length`` letters
(``split_monostring`` below: the reference's ``MonoString.split``, with what that method does to ``mono2nucl``); and gaps are filled from the
higher-order repeat: the HOR is the contig of the de Bruijn graph on the frequent 3-mers — counted on the device,
``Engine.monokmers`` — and a window of the HOR's length whose known letters all agree with the HOR, with at least one gap and at
most ``max_gap`` of them, takes the HOR's letters.  ``correct_gaps`` keeps the reference's sequential, in-place rule: per read the
HORs in sorted order, 1 .. nhor copies, windows left to right, and a filled window changes what the later ones see.  A fill never
changes a known letter, so a window that disagrees with the HOR now never agrees later: the windows that agree are found in one
vectorised pass and only those are looked at again, in order, with their gap count of that moment (with nhor = 2 a fill can
bring an overlapping later window's gaps DOWN to max_gap, so the count cannot be taken once).  No networkx, no Biopython."""
from collections import Counter
from copy import deepcopy

import numpy as np

from .debruijn_graph import DeBruijnGraph, get_frequent_kmers
from .sd_parser import MonoString, get_stats


def min_cyclic_shift(s):
    """the smallest rotation of s"""
    return min((s + s)[i:i + len(s)] for i in range(len(s)))


def split_monostring(monostring, c, min_length):
    """The reference's ``MonoString.split(c, min_length)`` as a function (the class in sd_parser.py stays as it is): the pieces
    between the symbols c that have at least min_length letters, as {(name, piece number): MonoString}.  Equal to the reference's
    method AS IT BEHAVES: its inner loop bounds a position by the length of the piece, not by where the piece ends,
    and has no end-of-list test, so pieces behind the first get a truncated or empty mono2nucl and some strings raise IndexError."""
    pieces = {}
    keys = list(monostring.mono2nucl)      # in the dict's own order: descending after check_reverse
    at = 0                                 # never goes back
    begin = 0                              # where the piece starts in the string
    for number, piece in enumerate(monostring.tostring().split(c)):
        if len(piece) >= min_length:
            while at < len(keys) and keys[at] < begin:
                at += 1
            taken = {}
            while keys[at] < len(piece):      # the reference's bound and its missing end test: IndexError past the last key
                coord = keys[at]
                assert piece[coord - begin] == monostring.mono2nucl[coord][0]
                taken[coord - begin] = monostring.mono2nucl[coord]
                at += 1
            part = MonoString(name=monostring.name, string=list(piece), mono2nucl=taken, gap_symb=monostring.gap_symb, strand=monostring.strand)
            reference_validity(part)
            pieces[(monostring.name, number)] = part
        begin += len(piece) + 1
    return pieces


def reference_validity(monostring):
    """The reference's own validity check, as it behaves on the parts of the split: it reports a negative coordinate and then indexes
    with it, and stumbles over a misspelt attribute at a coordinate past the end (``MonoString.assert_validity`` is stricter)."""
    for coord, (letter, _, _) in monostring.mono2nucl.items():
        if coord < 0:
            print(coord, letter)
        if coord >= len(monostring.string):
            raise AttributeError("'MonoString' object has no attribute 'stirng'")
        assert letter == monostring.string[coord]


def get_ma(x, N):
    """the moving average of x over windows of N (empty when x is shorter than N)"""
    run = np.cumsum(np.insert(x, 0, 0))
    return (run[N:] - run[:-N]) / float(N)


def filter_lowercaserich_reads(monoreads, max_lowercase=0.1):
    kept = {}
    for r_id, read in monoreads.items():
        if np.mean([c.islower() for c in read]) <= max_lowercase:      # (an empty read has no mean: it goes)
            kept[r_id] = read
    return kept


def trim_read(monoread, max_gap, ma_window, gap_symb='?'):
    ma = get_ma([c == gap_symb for c in monoread], N=ma_window)
    good = np.nonzero(~(ma > max_gap))[0]
    left, right = (int(good[0]), int(good[-1])) if len(good) else (len(ma), -1)
    monoread.trim_read(left, right + ma_window + 1)
    monoread.strip()
    return monoread


def trim_reads(monoreads, max_gap=0.2, ma_window=30):
    return {r_id: trim_read(read, max_gap=max_gap, ma_window=ma_window) for r_id, read in monoreads.items()}


def cut_gaprich_reads(monoreads, max_gap=0.05, min_length=100, gap_symb='?'):
    out = {}
    n_cut = n_parts = 0
    for r_id, read in monoreads.items():
        if len(read) == 0:
            out[r_id] = read
        elif Counter(read)[gap_symb] / len(read) <= max_gap:
            out[(r_id, 0)] = read
        else:
            parts = split_monostring(read, c=gap_symb, min_length=min_length)
            filled = sum(len(part.string) > 0 for part in parts.values())
            if filled:
                n_cut += 1
                n_parts += filled
            out.update(parts)
    return out, n_cut, n_parts


def _fill_from(monostring, hor, max_gap, gap_symb):
    """windows left to right; only those whose known letters agree with hor can ever be filled"""
    n, m = len(monostring), len(hor)
    if n < m:
        return
    letters = monostring.string
    if any(len(c) != 1 for c in letters) or len(gap_symb) != 1:
        starts = range(n - m + 1)
    else:
        arr = np.array([ord(c) for c in letters], np.int64)
        gap = ord(gap_symb)
        agree = np.ones(n - m + 1, bool)
        for j, h in enumerate(hor):
            col = arr[j:j + n - m + 1]
            agree &= (col == ord(h)) | (col == gap)
        starts = np.nonzero(agree)[0].tolist()
    for i in starts:
        window = letters[i:i + m]
        gaps = window.count(gap_symb)
        if gaps == 0 or gaps / m > max_gap:
            continue
        if all(x == gap_symb or x == y for x, y in zip(window, hor)):
            letters[i:i + m] = list(hor)


def correct_gaps(monostrings, max_gap=0.3, nhor=1, k=3, min_mult=5000, gap_symb='?'):
    frequent_kmers, _ = get_frequent_kmers(monostrings, k=k, min_mult=min_mult)
    db = DeBruijnGraph(k=k)
    db.add_kmers(frequent_kmers, coverage=frequent_kmers)
    hors, _ = db.get_contigs()
    hors = sorted(min_cyclic_shift(hor) for hor in hors)
    for monostring in monostrings.values():
        for single in hors:
            for copies in range(1, nhor + 1):
                _fill_from(monostring, single * copies, max_gap, gap_symb)
        reference_validity(monostring)
    return monostrings


def error_correction(monoreads, inplace=True, verbose=False, hor_correction=True):
    if not inplace:
        monoreads = deepcopy(monoreads)

    def report(title, reads):
        if verbose:
            print(title)
            get_stats(reads, verbose=True, return_stats=False)

    report('Stats for uncorrected reads', monoreads)
    reads = filter_lowercaserich_reads(monoreads)
    report('\nStats for filtered reads', reads)
    reads = trim_reads(reads)
    report('\nStats for trimmed+filtered reads', reads)
    reads, n_cut, n_parts = cut_gaprich_reads(reads)
    if verbose:
        print('\nStats for cut_gaprich_reads+trimmed+filtered reads')
        print(f'# cut reads = {n_cut}')
        print(f'# total cut parts = {n_parts}')
        get_stats(reads, verbose=True, return_stats=False)
    if hor_correction:
        reads = correct_gaps(reads)
        report('\nStats for hor_corrected+cut_gaprich_reads+trimmed+filtered reads', reads)
    return reads

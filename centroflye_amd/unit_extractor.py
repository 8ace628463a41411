"""The HOR period and unit of raw reads: mirror of the reference's ``scripts/unit_extractor.py``.

The reference walks one read at a time through Python dicts (:23-103).  Here ``extract_units`` sends every read of the input through
``Engine.tandem_scan`` in one batch (cf_tandem.hip: period, best distance window, hook k-mer and the hook's positions) and does
only rule 5 on the host: cut the read at the hook, pick the ``median_high`` piece, write the two files per read.

The functions with the reference's names are plain host code with the reference's results for ANY string, kept for API parity and
for the reads the device hands back (status "exotic": a window with N, lower case or another byte is a k-mer of its own for the
reference, which compares raw substrings, while the device only codes upper-case ACGT).

Defined here, not by the reference: a read without a repeated k-mer gets the status "no period" and no directory (the reference
raises on ``periods[0]``); nothing runs Flye and nothing is plotted unless asked for; two reads whose ids share their first 8
characters still share a directory, the later one wins, and a warning names both (``full_ids`` uses the whole id); a duplicate id is
an error before anything is written; ``periods.tsv`` is new.
"""
import os
import statistics
import subprocess
import sys
from bisect import bisect_left, bisect_right

import numpy as np

from .read_recruitment import iter_seqs

STATUS = ("ok", "no_period", "exotic")
TSV_COLUMNS = ("id", "status", "length", "rep_kmers", "distances", "period", "bin_left", "bin_right", "count", "hook", "hook_index",
               "pieces", "med_len", "template")


# ---------------------------------------------------------------------------------------------- the reference's functions
def get_repetitive_kmers(seq, k):
    """{k-mer: [start positions]} of the k-mers with two or more positions, in order of first occurrence (:23-30)."""
    where = {}
    for i in range(len(seq) - k + 1):
        where.setdefault(seq[i:i + k], []).append(i)
    return {kmer: pos for kmer, pos in where.items() if len(pos) >= 2}


def get_convolution(rep_kmers):
    """({k-mer: sorted differences of consecutive positions}, all of them sorted) (:33-40)."""
    conv = {kmer: sorted(b - a for a, b in zip(pos, pos[1:])) for kmer, pos in rep_kmers.items()}
    union = sorted(d for dist in conv.values() for d in dist)
    return conv, union


def get_period_info(conv, bin_size):
    """(periods, bin_convs, bin_left, bin_right) of a sorted distance list (:43-78): the windows conv[l:r(l)] with r(l) the first index
    beyond conv[l] + 2 bin_size, for l = 0, 1, .. up to the first one that reaches the end.  bin_left / bin_right are the ends of the
    FIRST window with the most distances.  periods / bin_convs pair every surviving count with a window median, largest count first,
    through the reference's two dicts: a count maps to the median of the last window that brought a new median or a larger count
    for a known one, and a median that moves to a larger count drops the entry of its old count — whichever median owns it by then.
    An empty list gives ([], [], None, None)."""
    n = len(conv)
    if n == 0:
        return [], [], None, None
    count_of, period_of = {}, {}      # median -> its largest count so far; count -> the median entered last
    best = (0, 0)
    l = r = 0
    while r < n:
        while r < n and conv[r] - conv[l] <= 2 * bin_size:
            r += 1
        count, mid = r - l, l + (r - l) // 2
        period = conv[mid] if count % 2 else (conv[mid] + conv[mid - 1]) // 2
        known = count_of.get(period)
        if known is None or count > known:
            period_of[count] = period
            if known is not None:
                period_of.pop(known, None)
            count_of[period] = count
        if count > best[1] - best[0]:
            best = (l, r)
        l += 1
    order = sorted(period_of.items(), reverse=True)
    return tuple(p for _, p in order), tuple(c for c, _ in order), conv[best[0]], conv[best[1] - 1]


def get_hook_kmer(conv, bin_left, bin_right):
    """The k-mer with the most distances inside [bin_left, bin_right], the first such k-mer of the dict on a tie; None when no
    k-mer has one (:81-89)."""
    hook, most = None, 0
    for kmer, dist in conv.items():
        inside = bisect_right(dist, bin_right) - bisect_left(dist, bin_left)
        if inside > most:
            hook, most = kmer, inside
    return hook


def hook_positions(seq, hook):
    """Every start of the hook in seq, overlapping ones included."""
    pos, i = [], seq.find(hook)
    while i >= 0:
        pos.append(i)
        i = seq.find(hook, i + 1)
    return pos


def splits_from_positions(seq, pos):
    return {f"split_{s}_{e}": seq[s:e] for s, e in zip(pos, pos[1:])}


def split_by_hook(seq, hook):
    """{'split_<s>_<e>': seq[s:e]} for consecutive hook positions, in order of s (:92-103)."""
    return splits_from_positions(seq, hook_positions(seq, hook))


def select_template(splits):
    """(med_len, template id): median_high of the pieces' lengths and the first id in STRING order whose piece has it (:121-129)."""
    med_len = statistics.median_high([len(s) for s in splits.values()])
    for split_id in sorted(splits):
        if len(splits[split_id]) == med_len:
            return med_len, split_id
    raise AssertionError("median_high is one of the lengths")


# ---------------------------------------------------------------------------------------------- per-read result
class ReadResult:
    __slots__ = ("id", "status", "length", "n_rep_kmers", "n_conv", "period", "bin_left", "bin_right", "count", "hook", "hook_index",
                 "hook_pos", "on_host")

    def __init__(self, seq_id, length):
        self.id, self.length = seq_id, length
        self.status, self.n_rep_kmers, self.n_conv = "no_period", 0, 0
        self.period = self.bin_left = self.bin_right = self.count = self.hook = None
        self.hook_index, self.hook_pos, self.on_host = 0, [], False


def scan_read_on_host(seq_id, seq, k, bin_size):
    """The reference's four functions on one read."""
    res = ReadResult(seq_id, len(seq))
    res.on_host = True
    rep = get_repetitive_kmers(seq, k)
    conv, union = get_convolution(rep)
    res.n_rep_kmers, res.n_conv = len(rep), len(union)
    if not union:
        return res
    periods, bin_convs, res.bin_left, res.bin_right = get_period_info(union, bin_size)
    res.status, res.period, res.count = "ok", periods[0], bin_convs[0]
    res.hook = get_hook_kmer(conv, res.bin_left, res.bin_right)
    dist = conv[res.hook]
    res.hook_index = bisect_right(dist, res.bin_right) - bisect_left(dist, res.bin_left)
    res.hook_pos = rep[res.hook]
    return res


def scan_reads(ids, seqs, k=15, bin_size=10, engine=None):
    """[ReadResult] for the reads (ids: str, seqs: str), the batch on the device and the exotic reads on the host."""
    from . import session
    from .engine import Engine
    if not 1 <= k <= 31:
        raise ValueError("k must lie in 1 .. 31")
    engine = engine or session.engine()      # raises without GPU / library: no fallback
    raw = [s.encode("latin-1") for s in seqs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(s) for s in raw], out=off[1:])
    rows = engine.tandem_scan(b"".join(raw), off, k, bin_size)
    ptr, pos = engine.tandem_hook_positions()
    out = []
    for i, (seq_id, seq) in enumerate(zip(ids, seqs)):
        row = rows[i]
        if row["status"] == Engine.TANDEM_EXOTIC:
            out.append(scan_read_on_host(seq_id, seq, k, bin_size))
            continue
        res = ReadResult(seq_id, len(seq))
        res.n_rep_kmers, res.n_conv = int(row["n_rep_kmers"]), int(row["n_conv"])
        if row["status"] == Engine.TANDEM_OK:
            res.status = "ok"
            res.period, res.bin_left, res.bin_right, res.count = (int(row[f]) for f in ("period", "bin_left", "bin_right", "count"))
            res.hook_index = int(row["hook_index"])
            res.hook = seq[int(row["hook_pos"]):int(row["hook_pos"]) + k]
            res.hook_pos = pos[ptr[i]:ptr[i + 1]].tolist()
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------- files
def write_seqs(path, seqs):
    with open(path, "w") as f:
        for seq_id, seq in seqs.items():
            f.write(f">{seq_id}\n{seq}\n")


def flye_argv(splits_fn, target_fn, outdir, flye_bin="flye", num_threads=50):
    """The reference's Flye call (:139-145)."""
    return [flye_bin, "--nano-raw", splits_fn, "--polish-target", target_fn, "-i", "2", "-t", str(num_threads), "-o", outdir]


def read_input(reads_path):
    """(ids, seqs) as str; the id is the first word of the header.  A duplicate id raises before anything is written."""
    ids, seqs, seen = [], [], set()
    for name, seq in iter_seqs(reads_path):
        seq_id = name.decode("latin-1")
        if seq_id in seen:
            raise ValueError(f"{reads_path}: the id {seq_id!r} occurs twice")
        seen.add(seq_id)
        ids.append(seq_id)
        seqs.append(seq.decode("latin-1"))
    return ids, seqs


def extract_units(reads_path, outdir, k=15, bin_size=10, engine=None, write_files=True, full_ids=False, polish=False, flye_bin="flye",
                  num_threads=50, plot=False, warn=None):
    """Every read of a FASTA / FASTQ(.gz) file: <outdir>/<id[:8]>/splits.fasta and median_read_unit.fasta as the reference writes
    them, and <outdir>/periods.tsv.  Returns the rows of periods.tsv as dicts (input order)."""
    warn = warn or (lambda msg: print(msg, file=sys.stderr))
    ids, seqs = read_input(reads_path)
    results = scan_reads(ids, seqs, k, bin_size, engine)
    if write_files:
        os.makedirs(outdir, exist_ok=True)
    rows, owner = [], {}
    for res, seq in zip(results, seqs):
        row = dict(id=res.id, status=res.status, length=res.length, rep_kmers=res.n_rep_kmers, distances=res.n_conv, period=res.period,
                   bin_left=res.bin_left, bin_right=res.bin_right, count=res.count, hook=res.hook, hook_index=res.hook_index, pieces=0,
                   med_len=None, template=None)
        rows.append(row)
        if res.status != "ok":
            continue
        splits = splits_from_positions(seq, res.hook_pos)
        row["pieces"] = len(splits)
        row["med_len"], row["template"] = select_template(splits)
        if not write_files:
            continue
        name = res.id if full_ids else res.id[:8]
        if name in owner:
            warn(f"warning: the reads {owner[name]!r} and {res.id!r} share the directory {name!r}: the later one wins")
        owner[name] = res.id
        read_outdir = os.path.join(outdir, name)
        os.makedirs(read_outdir, exist_ok=True)
        splits_fn, target_fn = os.path.join(read_outdir, "splits.fasta"), os.path.join(read_outdir, "median_read_unit.fasta")
        write_seqs(splits_fn, splits)
        write_seqs(target_fn, {row["template"]: splits[row["template"]]})
        if polish:
            subprocess.check_call(flye_argv(splits_fn, target_fn, read_outdir, flye_bin, num_threads))
        if plot:
            plot_convolution(seq, k, os.path.join(read_outdir, f"{name}.pdf"), name, res.period)
    if write_files:
        write_periods_tsv(os.path.join(outdir, "periods.tsv"), rows)
    return rows


def write_periods_tsv(path, rows):
    periods = [r["period"] for r in rows if r["status"] == "ok"]
    with open(path, "w") as f:
        f.write("#" + "\t".join(TSV_COLUMNS) + "\n")
        for r in rows:
            f.write("\t".join("." if r[c] is None else str(r[c]) for c in TSV_COLUMNS) + "\n")
        f.write(f"# median period of {len(periods)} reads: {statistics.median(periods) if periods else '.'}\n")


def plot_convolution(seq, k, path, name, period):
    """The reference's histogram (:148-151), when matplotlib is there; its bytes are never compared."""
    try:
        import matplotlib
        matplotlib.use("agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    _, union = get_convolution(get_repetitive_kmers(seq, k))
    plt.hist(union, bins=100)
    plt.title(f"Tandem read convolution, {name}, period={period}")
    plt.savefig(path, format="pdf")
    plt.close()
    return True


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="HOR period and unit of raw reads (the reference's scripts/unit_extractor.py)")
    ap.add_argument("-i", "--input", required=True, help="input reads (FASTA / FASTQ, plain or gzip)")
    ap.add_argument("-o", "--outdir", required=True, help="output directory")
    ap.add_argument("-k", type=int, default=15, help="k-mer length (1 .. 31)")
    ap.add_argument("-b", "--bin-size", type=int, default=10, help="bin size")
    ap.add_argument("--polish", action="store_true", help="run the reference's Flye command on every read's pieces")
    ap.add_argument("--flye-bin", default="flye")
    ap.add_argument("--num-threads", type=int, default=50)
    ap.add_argument("--plot", action="store_true", help="write the distance histogram of every read (needs matplotlib)")
    ap.add_argument("--full-ids", action="store_true", help="name a read's directory by its whole id, not its first 8 characters")
    p = ap.parse_args(argv)
    if not 1 <= p.k <= 31 or p.bin_size < 0:
        print("unit_extractor: k must lie in 1 .. 31 and the bin size must not be negative", file=sys.stderr)
        return 2
    try:
        rows = extract_units(p.input, p.outdir, p.k, p.bin_size, full_ids=p.full_ids, polish=p.polish, flye_bin=p.flye_bin,
                             num_threads=p.num_threads, plot=p.plot)
    except ValueError as e:
        print(f"unit_extractor: {e}", file=sys.stderr)
        return 1
    for r in rows:
        print(f"{r['id']}: {r['status']}" + (f", selected period = {r['period']}" if r["status"] == "ok" else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())

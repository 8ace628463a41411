"""The consensus length class over many reads' units: mirror of the reference's ``scripts/unit_clusterer.py`` (:19-78).  Host only.

Every sub-directory of the input holds one unit (``polished_2.fasta`` after the extractor's Flye run; ``--units-name
median_read_unit.fasta`` takes the extractor's own output with no Flye in between).  The sorted unit lengths go through the
extractor's ``get_period_info``; the units inside [bin_left, bin_right] are ``cluster_units.fasta``, and the first one in id
order whose length is ``statistics.median`` of theirs is ``median_read_unit.fasta`` — the file that goes to NCRF as the HOR unit.

Defined here, not by the reference: directories are taken in name order (the reference: scandir order); Flye runs only with
``polish``; where the reference raises (no directory; the median of an even number of lengths falling between two of them, so
that no unit has it) ``ClusterError`` names the cause and nothing is written.
"""
import os
import statistics
import subprocess
import sys

from .read_recruitment import iter_seqs
from .unit_extractor import flye_argv, get_period_info, write_seqs


class ClusterError(ValueError):
    pass


def get_units(input_dir, units_name="polished_2.fasta"):
    """{directory name: first sequence of its units file}, directories in name order."""
    units = {}
    for name in sorted(os.listdir(input_dir)):
        path = os.path.join(input_dir, name)
        if os.path.isdir(path):
            fn = os.path.join(path, units_name)
            if not os.path.isfile(fn):
                raise ClusterError(f"{fn} is missing")
            seq = next((s for _, s in iter_seqs(fn)), None)
            if seq is None:
                raise ClusterError(f"{fn} holds no sequence")
            units[name] = seq.decode("latin-1")
    return units


def select_median_seq(seqs):
    """(id, sequence, median length): the first id in string order whose length is statistics.median of all lengths (:29-38)."""
    median_len = statistics.median([len(s) for s in seqs.values()])
    for seq_id in sorted(seqs):
        if len(seqs[seq_id]) == median_len:
            return seq_id, seqs[seq_id], median_len
    raise ClusterError(f"the median length {median_len} of the {len(seqs)} clustered units falls between two lengths: no unit has it")


def cluster_units(input_dir, outdir, bin_size=50, units_name="polished_2.fasta", polish=False, flye_bin="flye", num_threads=50):
    """Writes cluster_units.fasta and median_read_unit.fasta; returns a dict of what was chosen."""
    units = get_units(input_dir, units_name)
    if not units:
        raise ClusterError(f"{input_dir} holds no directory with units")
    lens = sorted(len(u) for u in units.values())
    periods, bin_convs, bin_left, bin_right = get_period_info(lens, bin_size)
    cluster = {name: u for name, u in units.items() if bin_left <= len(u) <= bin_right}
    median_id, median_unit, median_len = select_median_seq(cluster)      # (raises before anything is written)
    os.makedirs(outdir, exist_ok=True)
    cluster_fn, median_fn = os.path.join(outdir, "cluster_units.fasta"), os.path.join(outdir, "median_read_unit.fasta")
    write_seqs(cluster_fn, cluster)
    write_seqs(median_fn, {median_id: median_unit})
    if polish:
        subprocess.check_call(flye_argv(cluster_fn, median_fn, outdir, flye_bin, num_threads))
    return dict(n_units=len(units), n_cluster=len(cluster), bin_left=bin_left, bin_right=bin_right, periods=list(periods),
                bin_convs=list(bin_convs), median_id=median_id, median_len=median_len)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="consensus length class of read units (the reference's scripts/unit_clusterer.py)")
    ap.add_argument("-i", "--input", required=True, help="directory with one sub-directory per read")
    ap.add_argument("-o", "--outdir", required=True, help="output directory")
    ap.add_argument("-b", "--bin-size", type=int, default=50, help="bin size")
    ap.add_argument("--units-name", default="polished_2.fasta", help="the units file inside every sub-directory")
    ap.add_argument("--polish", action="store_true", help="run the reference's Flye command on the cluster")
    ap.add_argument("--flye-bin", default="flye")
    ap.add_argument("--num-threads", type=int, default=50)
    p = ap.parse_args(argv)
    try:
        if not os.path.isdir(p.input):
            raise ClusterError(f"{p.input} is not a directory")
        got = cluster_units(p.input, p.outdir, p.bin_size, p.units_name, p.polish, p.flye_bin, p.num_threads)
    except ClusterError as e:
        print(f"unit_clusterer: {e}", file=sys.stderr)
        return 1
    print(f"{got['n_cluster']} of {got['n_units']} units in [{got['bin_left']}, {got['bin_right']}]; median unit {got['median_id']} ({got['median_len']} bases)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

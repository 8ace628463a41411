"""Shared by the tandem (unit extractor) tests and tests/golden/make_golden_tandem.py: the seeded inputs, a numpy statement of the
reference's rules (scripts/unit_extractor.py:23-136) that shares no code with centroflye_amd/unit_extractor.py, planted
misreadings of those rules (WRONG_RULES: the goldens must tell every one of them from the reference), and the comparison of an
Engine's answers with the recorded ones."""
import hashlib
import json
import os
import statistics

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tandem_cases.json")
SHAPE = dict(sort_tile=4096, rec_tile=2048, scan_tile=2048, block=256)      # the borders the "tiles" case is built around

WRONG_RULES = ("period_of_best_l", "strict_less_at_two_bins", "upper_middle_for_even", "last_best_window", "open_hook_interval",
               "hook_tie_to_smaller_kmer", "run_joined_across_reads", "template_by_numeric_order", "median_low")


def sha(data):
    return hashlib.sha256(data if isinstance(data, (bytes, bytearray)) else bytes(data)).hexdigest()


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- inputs
def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def mutate(rng, seq, rate, indel_share=2 / 3):
    """Errors at `rate` per base: deletions and insertions, half of indel_share each, substitutions the rest."""
    out = bytearray()
    p_del, p_indel = rate * indel_share / 2, rate * indel_share
    for c in seq:
        u = rng.random()
        if u < p_del:                   # deletion
            continue
        if u < p_indel:                 # insertion in front of the base
            out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            out.append(c)
        elif u < rate:                  # substitution
            out.append(int(rng.choice([x for x in b"ACGT" if x != c])))
        else:
            out.append(c)
    return bytes(out)


def tandem_read(rng, unit, copies, rate, lead=0):
    return mutate(rng, rand_seq(rng, lead) + unit * copies, rate) if rate else rand_seq(rng, lead) + unit * copies


def hor_unit(rng, n_mono=12, total=2055):
    """A DXZ1-shaped HOR: n_mono monomers of about 171 bases, each the base monomer with a quarter of its bases changed."""
    base = rand_seq(rng, 171)
    lens = [171] * n_mono
    for i in range(total - 171 * n_mono):
        lens[i % n_mono] += 1
    unit = b""
    for ln in lens:
        m = bytearray(mutate(rng, base, 0.25))
        while len(m) < ln:
            m += rand_seq(rng, 1)
        unit += bytes(m[:ln])
    assert len(unit) == total
    return unit


def hor_reads(seed=11, n=64, length=20000, rate=0.10, total=2055):
    """64 reads of 20 kb off an array of one HOR, 10 % errors: 8 % substitutions, 1 % insertions, 1 % deletions.  All distances between
    two neighbouring copies share those copies' net indel, whose standard deviation is sqrt(2055 x 0.02) = 6.4 bases here; with a
    third of the errors each it is 11.7, more than the bin size of 10, and the reference's own period leaves 2055 +- 10 on reads
    of nine copies."""
    rng = np.random.default_rng(seed)
    unit = hor_unit(rng, total=total)
    array = unit * (length // total + 3)
    reads = []
    for i in range(n):
        s = int(rng.integers(0, total))
        reads.append(mutate(rng, array[s:s + length + 1500], rate, 0.2)[:length])
    return reads


def _ids(prefix, n):
    return [f"{prefix}{i:03d}" for i in range(n)]      # at most 7 characters: no two share their first 8


def cases():
    """[dict(name, k, bin_size, ids, reads)]: the smallest shapes at which the rules and the kernels can go wrong."""
    out = []

    def add(name, k, bin_size, reads, ids=None):
        out.append(dict(name=name, k=k, bin_size=bin_size, reads=list(reads), ids=ids or _ids(name[:4], len(reads))))

    rng = np.random.default_rng(5)
    add("no_reads", 15, 10, [])
    # shorter than k, exactly k, k + 1 without and with a repeat (n_conv = 1), an empty read
    add("lengths_around_k", 4, 10, [b"ACG", b"ACGT", b"ACGTA", b"AAAAA", b"", b"ACGTTACGT"])
    add("no_repeat", 15, 10, [rand_seq(rng, 300)])
    one = rand_seq(rng, 40)
    add("one_repeat", 15, 10, [one + rand_seq(rng, 23) + one[:15] + rand_seq(rng, 9)])
    unit37 = rand_seq(rng, 37)
    add("perfect_tandem", 15, 10, [unit37 * 12, rand_seq(rng, 50) + unit37 * 7])
    add("homopolymer", 5, 10, [b"A" * 100, b"AAAAAACCCCCCCC" * 3])
    noisy = [tandem_read(rng, rand_seq(rng, int(rng.integers(20, 70))), int(rng.integers(5, 14)), float(rng.uniform(0.03, 0.15)),
                         int(rng.integers(0, 30))) for _ in range(48)]
    add("bin_size_0", 7, 0, noisy[:16])
    add("noisy_k6_bin3", 6, 3, noisy)
    add("noisy_k8_bin2", 8, 2, noisy[:24])
    short = [tandem_read(rng, rand_seq(rng, int(rng.integers(5, 12))), int(rng.integers(4, 9)), 0.08) for _ in range(12)]
    for k in (1, 15, 16, 31):
        add(f"k_{k}", k, 4, short + noisy[:6] + [tandem_read(rng, rand_seq(rng, 90), 6, 0.02)])
    # the same k-mer (and nothing else) last in read i and first in read i + 1; it occurs once in each
    x = rand_seq(rng, 15)
    add("read_border", 15, 10, [rand_seq(rng, 60) + x, x + rand_seq(rng, 60), x + rand_seq(rng, 30) + x, rand_seq(rng, 20) + x])
    # one (read, k-mer) run and one read's distances across every tile border of SHAPE: homopolymers of 2 996 windows back to back
    add("tiles", 5, 10, [b"A" * 3000, b"C" * 3000, tandem_read(rng, rand_seq(rng, 50), 40, 0.0), b"G" * 3000,
                         tandem_read(rng, rand_seq(rng, 41), 30, 0.05), b"T" * 2600])
    # N runs and a soft-masked stretch that repeats, next to plain reads
    u = rand_seq(rng, 60)
    soft = u[:20] + u[20:45].lower() + u[45:]
    add("exotic", 15, 10, [soft * 6, tandem_read(rng, u, 6, 0.05), u * 2 + b"N" * 40 + u * 3 + b"N" * 40 + u, b"N" * 50,
                           (u[:30] + b"NNNNNNNNNNNNNNNNNNNN" + u[30:]) * 5])
    add("hor64", 15, 10, hor_reads())
    return out


def cluster_cases():
    """[(name, bin_size, {directory name: unit})] for the clusterer: odd and even clusters, an outlier class, a median between two
    lengths (the reference raises), one unit, bin size 0, two classes of equal size."""
    rng = np.random.default_rng(21)

    def units(lens):
        return {f"read{i:04d}": rand_seq(rng, n).decode() for i, n in enumerate(lens)}
    return [("odd_cluster", 50, units([2055, 2057, 2049, 2060, 2051, 4110, 171, 2058, 2044])),
            ("even_cluster_shared_median", 50, units([2055, 2055, 2049, 2060, 1000, 3000])),
            ("median_between_two_lengths", 50, units([2050, 2056, 2040, 2061, 171])),
            ("one_unit", 50, units([2055])),
            ("bin_size_0", 0, units([100, 100, 100, 101, 99, 100])),
            ("two_classes_first_wins", 5, units([100, 101, 102, 200, 201, 202, 300]))]


# ---------------------------------------------------------------------------------------------- the rules, in numpy
def _windows(seq, k):
    """(ids of the distinct windows by first occurrence, positions) or None."""
    n = len(seq) - k + 1
    if n < 1:
        return None
    a = np.frombuffer(seq, np.uint8)
    rows = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(a, k))
    _, first, inv = np.unique(rows.view(np.dtype((np.void, k))).ravel(), return_index=True, return_inverse=True)
    return first[inv.ravel()], first      # a window's id = the position of its first occurrence


def restate(seq, k, bin_size, wrong=None, extra=None):
    """The rules 1-5 for one read (bytes).  extra: {first position: [distances]} added by the batch-level misreading."""
    res = dict(n_rep_kmers=0, n_conv=0, period=None, count=None, bin_left=None, bin_right=None, hook_pos=None, hook_index=0,
               positions=[], split_ids=[], med_len=None, template=None)
    w = _windows(seq, k)
    if w is None:
        return res
    ids, _ = w
    pos = np.arange(ids.size)
    order = np.lexsort((pos, ids))
    sid, spos = ids[order], pos[order]
    same = sid[1:] == sid[:-1]
    d_id, d = sid[1:][same], (spos[1:] - spos[:-1])[same]
    if extra:
        d_id = np.concatenate([d_id, np.repeat(list(extra), [len(v) for v in extra.values()])]).astype(np.int64)
        d = np.concatenate([d, [x for v in extra.values() for x in v]]).astype(np.int64)
    res["n_rep_kmers"], res["n_conv"] = int(np.unique(d_id).size), int(d.size)
    if d.size == 0:
        return res
    conv = np.sort(d)
    n = conv.size
    r = np.searchsorted(conv, conv + 2 * bin_size, "left" if wrong == "strict_less_at_two_bins" else "right")
    r = np.maximum(r, np.arange(n) + 1)
    visited = int(np.argmax(r == n)) + 1
    l = np.arange(visited)
    count = r[:visited] - l
    mid = l + count // 2
    period = np.where((count % 2 == 1) | (wrong == "upper_middle_for_even"), conv[mid], (conv[mid] + conv[np.maximum(mid - 1, 0)]) // 2)
    C = int(count.max())
    best = np.flatnonzero(count == C)
    best_l = int(best[-1] if wrong == "last_best_window" else best[0])
    bl, br = int(conv[best_l]), int(conv[r[best_l] - 1])
    if wrong == "period_of_best_l":
        p0 = int(period[best_l])
    else:
        first_l = {}
        for i in best:
            first_l.setdefault(int(period[i]), int(i))
        p0 = max(first_l, key=first_l.get)
    res.update(period=p0, count=C, bin_left=bl, bin_right=br, n_windows=visited)
    inside = (d > bl) & (d < br) if wrong == "open_hook_interval" else (d >= bl) & (d <= br)
    kmers, index = np.unique(d_id[inside], return_counts=True)
    if kmers.size == 0:
        return res
    top = kmers[index == index.max()]
    if wrong == "hook_tie_to_smaller_kmer":
        hook_pos = int(min(top, key=lambda p: seq[p:p + k]))
    else:
        hook_pos = int(top.min())
    hook = seq[hook_pos:hook_pos + k]
    positions = [i for i in range(len(seq) - k + 1) if seq[i:i + k] == hook]
    res.update(hook_pos=hook_pos, hook_index=int(index.max()), positions=positions)
    pieces = [(s, e) for s, e in zip(positions, positions[1:])]
    if not pieces:      # (only a misreading gets here: the hook has a distance, so two positions)
        return res
    lens = [e - s for s, e in pieces]
    med = statistics.median_low(lens) if wrong == "median_low" else statistics.median_high(lens)
    names = [f"split_{s}_{e}" for s, e in pieces]
    ranked = names if wrong == "template_by_numeric_order" else sorted(names)
    res.update(split_ids=names, med_len=med, template=next(x for x in ranked if int(x.split("_")[2]) - int(x.split("_")[1]) == med))
    return res


def restate_case(case, wrong=None):
    reads, k = case["reads"], case["k"]
    out = []
    for i, seq in enumerate(reads):
        extra = None
        if wrong == "run_joined_across_reads" and i > 0:
            # the last window of the read before and the first of this one hold the same k-mer: one run, one distance more
            before = reads[i - 1]
            if len(before) >= k and len(seq) >= k and before[-k:] == seq[:k]:
                extra = {0: [len(before) - k]}
        out.append(restate(seq, k, case["bin_size"], None if wrong == "run_joined_across_reads" else wrong, extra))
    return out


def files_of(seq, res):
    """(splits.fasta, median_read_unit.fasta) as bytes, from a restate() result."""
    splits = b"".join(b">" + x.encode() + b"\n" + seq[int(x.split("_")[1]):int(x.split("_")[2])] + b"\n" for x in res["split_ids"])
    t = res["template"]
    return splits, b">" + t.encode() + b"\n" + seq[int(t.split("_")[1]):int(t.split("_")[2])] + b"\n"


def summary(seq, res, k):
    """What the golden records of a read, from a restate() result (the golden maker builds the same dict from the reference)."""
    if res["period"] is None:
        return dict(n_rep_kmers=res["n_rep_kmers"], n_conv=res["n_conv"], period=None)
    if res["hook_pos"] is None or res["template"] is None:      # (only a misreading gets here: the best window holds a distance of some k-mer)
        return dict(n_rep_kmers=res["n_rep_kmers"], n_conv=res["n_conv"], period=res["period"], count=res["count"], hook=None)
    a, b = files_of(seq, res)
    return dict(n_rep_kmers=res["n_rep_kmers"], n_conv=res["n_conv"], period=res["period"], count=res["count"], bin_left=res["bin_left"],
                bin_right=res["bin_right"], n_windows=res["n_windows"], hook=seq[res["hook_pos"]:res["hook_pos"] + k].decode("latin-1"),
                hook_index=res["hook_index"], n_splits=len(res["split_ids"]), split_ids_sha=sha("\n".join(res["split_ids"]).encode()),
                med_len=res["med_len"], template=res["template"], splits_sha=sha(a), median_sha=sha(b))


COMPARED = ("n_rep_kmers", "n_conv", "period", "count", "bin_left", "bin_right", "hook", "hook_index", "n_splits", "split_ids_sha", "med_len", "template",
            "splits_sha", "median_sha")


def differs(rec, got):
    return any(rec.get(f) != got.get(f) for f in COMPARED)


# ---------------------------------------------------------------------------------------------- an Engine against the goldens
def pack(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(s) for s in reads], out=off[1:])
    return b"".join(reads), off


def is_exotic(seq, k):
    return len(seq) >= k and any(c not in b"ACGT" for c in seq)


def check_case(eng, G, case, expect_mode=None):
    """Runs one case through tandem_scan / tandem_hook_positions and compares every read with the recorded reference."""
    g = G["cases"][case["name"]]
    reads, k = case["reads"], case["k"]
    data, off = pack(reads)
    assert sha(data) == g["sha_in"], case["name"]
    rows = eng.tandem_scan(data, off, k, case["bin_size"])
    ptr, pos = eng.tandem_hook_positions()
    assert rows.size == len(reads) and ptr.size == len(reads) + 1 and ptr[0] == 0 and ptr[-1] == pos.size
    if expect_mode is not None and reads:
        assert eng.tandem_info()["key_mode"] == expect_mode
    for i, (seq, rec) in enumerate(zip(reads, g["reads"])):
        row, where = rows[i], f"{case['name']} read {i}"
        if is_exotic(seq, k):
            assert row["status"] == 2, where
            continue
        if rec["period"] is None:
            assert row["status"] == 1 and row["n_conv"] == 0 and row["n_rep_kmers"] == 0 and row["hook_pos"] == -1 and ptr[i] == ptr[i + 1], where
            continue
        assert row["status"] == 0, where
        got = {f: int(row[f]) for f in ("n_rep_kmers", "n_conv", "period", "count", "bin_left", "bin_right")}
        assert got == {f: rec[f] for f in got}, where
        assert seq[row["hook_pos"]:row["hook_pos"] + k].decode() == rec["hook"] and row["hook_index"] == rec["hook_index"], where
        p = pos[ptr[i]:ptr[i + 1]].tolist()
        assert row["n_hook"] == len(p) == rec["n_splits"] + 1 and p[0] == row["hook_pos"], where
        names = [f"split_{s}_{e}" for s, e in zip(p, p[1:])]
        assert sha("\n".join(names).encode()) == rec["split_ids_sha"], where
        assert row["n_windows"] == rec["n_windows"], where
    return rows

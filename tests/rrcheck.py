"""cf_rr_distances (cf_recruit.hip) at the limits of its launch shape: the seeded case generators and the case bodies shared by
the emulator and the GPU suite (test_emu_rr.py, test_gpu_rr.py).

The kernel gives one wave to every (read, strand) item, lane i owning block i (64 rows) of the unit; a wave takes items from a
ticket until they run out, and the grid is capped at 8 x n_cu workgroups of 4 waves.  The bodies below go where that shape can
go wrong:
  a  block counts       units of 1 .. 4096 bases (1 .. 64 blocks, the last lane included), the refusals around them
  b  chunk borders      the text loop's 64-step chunks: n_steps = L + nb - 1 around the multiples of 64, a last chunk of one step
  c  threshold edge     k = d, d - 1, -1 and m + 1 for reads whose distance d is known
  d  empty reads        in the middle of a batch (this repository's definition: all m bases of the unit inserted)
  e  more items than launched waves: 48 x n_cu + 37 reads in one call, and exactly 16 x n_cu
  f  the command line   scripts/rr.py on as many reads
Every expected distance of a - d is the REFERENCE's (vendored edlib, mode HW), stored as integers in tests/golden/rr_limits.json by
tests/golden/make_golden_rr.py from the generators here; e and f keep their units at 130 bases or fewer and take oracle.rr, the
plain-C restatement that tests/test_read_recruitment.py pins to the reference in that range.  Nothing compares the kernel with
itself.  All comparisons are integer-exact."""
import json
import os
import random

import numpy as np

from oracle import rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rr_limits.json")

BLOCK_UNITS = (1, 63, 64, 65, 2055, 3009, 4031, 4032, 4033, 4095, 4096)      # 1, 1, 1, 2, 33, 48, 63, 63, 64, 64, 64 blocks
BLOCK_THRESHOLDS = (-1, 40)
CHUNK_UNITS = (37, 100, 2055, 4096)                                          # nb = 1, 2, 33, 64
CHUNK_THRESHOLDS = (-1, 0)
EDGE_UNITS = (5, 64, 65, 130, 4096)
MANY_UNITS = (5, 64, 65, 130)
MANY_LENGTHS = lambda m: (0, 1, 2, m - 1, m, m + 1, 63, 64, 65, 127, 128, 129)      # noqa: E731


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def pack(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), off


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choices(alphabet, k=n))


def n_blocks(m):
    return (m + 63) // 64


# ------------------------------------------------------------------ a. block counts
def block_cases():
    """One (unit, reads) per unit length of BLOCK_UNITS: the unit inside random flanks, the reverse complement with a 3-base
    insertion in the middle, one base, the unit without its first and last 5 bases, an unrelated read of m + 63 bases, the bare
    unit, one read over ACGTacgtN."""
    rng = random.Random(4096)
    out = []
    for m in BLOCK_UNITS:
        unit = _seq(rng, m)
        rc = rr.revcomp(unit)
        flank = min(m + 30, 2100)
        reads = [_seq(rng, rng.randint(1, flank)) + unit + _seq(rng, rng.randint(1, flank)),
                 _seq(rng, 11) + rc[:m // 2] + _seq(rng, 3) + rc[m // 2:] + _seq(rng, 70),
                 _seq(rng, 1),
                 unit[5:-5] if m > 10 else unit[:1],
                 _seq(rng, m + 63),
                 unit,
                 _seq(rng, m // 2 + 9, b"ACGTacgtN")]
        out.append((unit, reads))
    return out


# ------------------------------------------------------------------ b. chunk borders of the text loop
def chunk_steps(m):
    """The values of n_steps = L + nb - 1 a unit of m bases is tried at: 63 .. 129 as they stand, and the same residues at the
    first multiple of 64 that leaves room for a whole copy of the unit and a flank (the + 1 of it is a last chunk of one step)."""
    q = -(-(m + n_blocks(m) + 64) // 64) * 64
    return sorted({63, 64, 65, 127, 128, 129, q - 1, q, q + 1, q + 63, q + 64, q + 65})


def chunk_cases():
    """Per unit of CHUNK_UNITS: for every n_steps of chunk_steps, a read of L = n_steps - nb + 1 bases that ends in an exact copy
    of the unit (the minimum is found in the very last step of the last lane) and one that starts with it — where L < m, the last
    and the first L bases of the unit; then L = m - 1, m, m + 1 as a deletion, a substitution and an insertion in the middle."""
    rng = random.Random(6463)
    out = []
    for m in CHUNK_UNITS:
        unit = _seq(rng, m)
        nb = n_blocks(m)
        reads, steps = [], []
        for n_steps in chunk_steps(m):
            L = n_steps - nb + 1
            if L < 1:
                continue
            if L >= m:
                reads += [_seq(rng, L - m) + unit, unit + _seq(rng, L - m)]
            else:
                reads += [unit[m - L:], unit[:L]]
            steps += [n_steps, n_steps]
        h = m // 2
        other = bytes([next(c for c in b"ACGT" if c != unit[h])])
        reads += [unit[:h] + unit[h + 1:], unit[:h] + other + unit[h + 1:], unit[:h] + other + unit[h:]]
        assert all(reads) and all(len(r) + nb - 1 == s for r, s in zip(reads, steps))
        out.append((unit, reads))
    return out


# ------------------------------------------------------------------ c. threshold edge
def edge_cases():
    """Per unit of EDGE_UNITS: the unit in flanks (d = 0), the unit under 1, m // 8 + 2 and m // 3 + 1 scattered substitutions in
    flanks, its reverse complement with two bases deleted, and an unrelated read (the unit of 4096 bases goes without the last
    of the substitution reads and the unrelated one: every read costs a call per threshold).  The thresholds come from the stored
    distances."""
    rng = random.Random(577)
    out = []
    for m in EDGE_UNITS:
        unit = _seq(rng, m)
        rc = rr.revcomp(unit)

        def hit(s, n):
            s = bytearray(s)
            for i in rng.sample(range(len(s)), min(n, len(s))):
                s[i] = next(c for c in b"ACGT" if c != s[i])
            return bytes(s)
        reads = [_seq(rng, 9) + unit + _seq(rng, 12)]
        reads += [_seq(rng, rng.randint(0, 40)) + hit(unit, n) + _seq(rng, rng.randint(0, 40)) for n in (1, m // 8 + 2, m // 3 + 1)[:3 if m < 4096 else 2]]
        reads += [_seq(rng, 20) + rc[:m // 3] + rc[m // 3 + 2:] + _seq(rng, 20), _seq(rng, m + 17)][:2 if m < 4096 else 1]
        out.append((unit, reads))
    return out


def edge_thresholds(m, ds):
    """-1, m + 1, and d and d - 1 for every distance d of ds (d - 1 only where it is a threshold: >= 0)."""
    return sorted({-1, m + 1} | {d for d in ds} | {d - 1 for d in ds if d >= 1})


def reference_limits(distance):
    """What tests/golden/rr_limits.json holds, computed with `distance(unit, read, k)`: integers only."""
    def both(unit, reads, k):
        rc = rr.revcomp(unit)
        return dict(fwd=[distance(unit, r, k) for r in reads], rc=[distance(rc, r, k) for r in reads])
    out = dict(blocks=[], chunks=[], edge=[])
    for name, cases, ks in (("blocks", block_cases(), BLOCK_THRESHOLDS), ("chunks", chunk_cases(), CHUNK_THRESHOLDS)):
        for unit, reads in cases:
            out[name].append(dict(m=len(unit), by_threshold={str(k): both(unit, reads, k) for k in ks}))
    for unit, reads in edge_cases():
        free = both(unit, reads, -1)
        ks = edge_thresholds(len(unit), free["fwd"] + free["rc"])
        out["edge"].append(dict(m=len(unit), thresholds=ks, by_threshold={str(k): both(unit, reads, k) for k in ks}))
    return out


def check_golden_is_sound(g):
    """Properties of the stored reference values themselves, so that a golden written from something else would not pass: the
    distances without limit are what the construction of the reads says, and a threshold only hides distances above it."""
    for name, cases in (("blocks", block_cases()), ("chunks", chunk_cases()), ("edge", edge_cases())):
        assert [c["m"] for c in g[name]] == [len(u) for u, _ in cases]
        for (unit, reads), c in zip(cases, g[name]):
            m = len(unit)
            free = c["by_threshold"]["-1"]
            for strand in ("fwd", "rc"):
                assert len(free[strand]) == len(reads) and all(max(0, m - len(r)) <= d <= m for r, d in zip(reads, free[strand]))
                for k, row in c["by_threshold"].items():
                    assert row[strand] == [d if int(k) < 0 or d <= int(k) else -1 for d in free[strand]], (name, m, k, strand)
    for c in g["blocks"]:
        f, r = c["by_threshold"]["-1"]["fwd"], c["by_threshold"]["-1"]["rc"]
        assert f[0] == 0 and f[5] == 0 and (c["m"] <= 10 or (f[3] == 10 and 1 <= r[1] <= 3)) and f[2] >= c["m"] - 1
    for (unit, reads), c in zip(chunk_cases(), g["chunks"]):
        free = c["by_threshold"]["-1"]["fwd"]
        assert free[:-3] == [max(0, c["m"] - len(r)) for r in reads[:-3]] and free[-3:] == [1, 1, 1]
    for c in g["edge"]:
        ds = c["by_threshold"]["-1"]["fwd"] + c["by_threshold"]["-1"]["rc"]
        assert c["thresholds"] == edge_thresholds(c["m"], ds) and c["by_threshold"]["-1"]["fwd"][0] == 0 and c["by_threshold"]["-1"]["fwd"][1] <= 1
        for strand in ("fwd", "rc"):
            for j, d in enumerate(c["by_threshold"]["-1"][strand]):      # the edge itself, spelt out per read
                assert c["by_threshold"][str(d)][strand][j] == d and c["by_threshold"][str(c["m"] + 1)][strand][j] == d
                assert d == 0 or c["by_threshold"][str(d - 1)][strand][j] == -1


def check_oracle_on_limits(g):
    """oracle.rr.distance (the plain-C restatement) against every stored reference value: pins it at 48 .. 64 blocks too.
    Returns how many distances were compared."""
    assert reference_limits(rr.distance) == g
    return sum(len(row[s]) for name in ("blocks", "chunks", "edge") for c in g[name] for row in c["by_threshold"].values() for s in row)


# ------------------------------------------------------------------ the bodies, each callable with any Engine
def _call(engine, unit, reads, k):
    flat, off = pack(reads)
    fwd, rc = engine.rr_distances(unit, flat, off, k)
    assert fwd.dtype == np.int32 and rc.dtype == np.int32 and fwd.size == len(reads) == rc.size
    return fwd.tolist(), rc.tolist()


def _check_stored(engine, cases, stored, what):
    n = 0
    for (unit, reads), c in zip(cases, stored):
        for k, want in c["by_threshold"].items():
            fwd, rc = _call(engine, unit, reads, int(k))
            assert fwd == want["fwd"], f"{what}: unit of {len(unit)} bases ({n_blocks(len(unit))} blocks), threshold {k}, forward"
            assert rc == want["rc"], f"{what}: unit of {len(unit)} bases ({n_blocks(len(unit))} blocks), threshold {k}, reverse complement"
            n += 2 * len(reads)
    return n


def check_block_counts(engine, g):
    """a.  Returns the number of distances compared."""
    from centroflye_amd.engine import DeviceError
    cases = block_cases()
    assert [n_blocks(len(u)) for u, _ in cases] == [1, 1, 1, 2, 33, 48, 63, 63, 64, 64, 64] and len(g["blocks"]) == len(cases)
    n = _check_stored(engine, cases, g["blocks"], "block counts")
    # units of 0 and 4097 bases are refused, and the same engine answers a unit of 4096 bases straight afterwards
    unit, reads = cases[-1]
    assert len(unit) == 4096
    for bad in (b"", unit + b"A"):
        try:
            _call(engine, bad, reads[:2], -1)
        except DeviceError as err:
            assert "(-22)" in str(err) and "1 .. 4096" in str(err)
        else:
            raise AssertionError(f"a unit of {len(bad)} bases was accepted")
        want = g["blocks"][-1]["by_threshold"]["40"]
        assert _call(engine, unit, reads, 40) == (want["fwd"], want["rc"]), f"after the refusal of a unit of {len(bad)} bases"
    return n


def check_chunk_borders(engine, g):
    """b.  Returns the number of distances compared."""
    cases = chunk_cases()
    assert [n_blocks(len(u)) for u, _ in cases] == [1, 2, 33, 64]
    for unit, reads in cases:
        steps = {len(r) + n_blocks(len(unit)) - 1 for r in reads}
        assert {s % 64 for s in steps} >= {63, 0, 1} and any(s % 64 == 1 and s > 64 for s in steps)
        assert {len(unit) - 1, len(unit), len(unit) + 1} <= {len(r) for r in reads}
    return _check_stored(engine, cases, g["chunks"], "chunk borders")


def check_threshold_edge(engine, g):
    """c.  Returns the number of distances compared."""
    cases = edge_cases()
    for c in g["edge"]:
        assert len(c["thresholds"]) >= 5 and set(map(str, c["thresholds"])) == set(c["by_threshold"])
    return _check_stored(engine, cases, g["edge"], "threshold edge")


def check_empty_reads_inside_a_batch(engine, g):
    """d.  The reads of a. for units of 65 and 4096 bases with empty reads between them, at the front and at the end: the others
    keep their stored answers; an empty read scores m, which is -1 under a threshold below m."""
    n = 0
    for (unit, reads), c in zip(block_cases(), g["blocks"]):
        m = len(unit)
        if m not in (65, 4096):
            continue
        mixed, where = [b""], []
        for i, r in enumerate(reads):
            where.append(len(mixed))
            mixed += [r] + [b""] * (i % 3)
        mixed.append(b"")
        for k, want in c["by_threshold"].items():
            k = int(k)
            empty = m if k < 0 or m <= k else -1
            fwd, rc = _call(engine, unit, mixed, k)
            for got, stored in ((fwd, want["fwd"]), (rc, want["rc"])):
                assert [got[i] for i in where] == stored, f"reads next to empty reads, unit of {m} bases, threshold {k}"
                assert [got[i] for i in range(len(mixed)) if i not in where] == [empty] * (len(mixed) - len(where))
            n += 2 * len(mixed)
    assert n
    return n


def near_palindrome(rng, m):
    """A unit that lies within m // 4 edits of its own reverse complement without being it: x + revcomp(x) (an odd length keeps a
    middle base) under m // 10 substitutions in the first half.  A read that holds the unit is then within the threshold of BOTH
    strands, at different distances."""
    x = _seq(rng, m // 2)
    unit = bytearray(x + _seq(rng, m % 2) + rr.revcomp(x))
    for i in rng.sample(range(m // 2), m // 10):
        unit[i] = next(c for c in b"ACGT" if c != unit[i])
    return bytes(unit)


def many_reads(m, unit, n, seed, n_long=5):
    """n reads for a unit of m bases: n_long of 20 000 bases at the front (their waves stay busy while the others go through many
    items), then every third read is the unit with one base deleted behind a 7-base flank and the others have a length drawn from
    MANY_LENGTHS(m) over ACGTN."""
    rng = np.random.default_rng(seed)
    acgtn = np.frombuffer(b"ACGTN", np.uint8)
    reads = [acgtn[rng.integers(0, 4, 20000)].tobytes() for _ in range(n_long)]
    lengths = MANY_LENGTHS(m)
    for i in range(n - n_long):
        if i % 3 == 0:
            cut = int(rng.integers(0, m))
            reads.append(acgtn[rng.integers(0, 4, 7)].tobytes() + unit[:cut] + unit[cut + 1:])
        else:
            reads.append(acgtn[rng.integers(0, 5, lengths[int(rng.integers(0, len(lengths)))])].tobytes())
    return reads


_MANY = {}


def many_reference(n_cu):
    """Units, reads and the oracle's answers of e. for a device of n_cu compute units, computed once per n_cu."""
    if n_cu in _MANY:
        return _MANY[n_cu]
    rng = random.Random(48)
    n = 48 * n_cu + 37
    out = []
    for m in MANY_UNITS:
        unit = near_palindrome(rng, m) if m > 5 else _seq(rng, m)
        rc = rr.revcomp(unit)
        assert unit != rc
        k = m // 4
        reads = many_reads(m, unit, n, 1000 + m)
        want = ([rr.distance(unit, r, k) for r in reads], [rr.distance(rc, r, k) for r in reads])
        # a kernel that answers -1 or m everywhere cannot pass: per strand a quarter within the threshold and a quarter not
        for strand in want:
            within = sum(d != -1 for d in strand)
            assert 4 * within >= n and 4 * (n - within) >= n, (m, within, n)
        assert want[0] != want[1]
        out.append(dict(unit=unit, k=k, reads=reads, want=want, within=[sum(d != -1 for d in s) for s in want]))
    _MANY[n_cu] = out
    return out


def check_more_items_than_waves(engine):
    """e.  48 x n_cu + 37 reads in one call (three items per launched wave, and a remainder), then exactly 16 x n_cu reads (one
    item per wave: the border of the launch cap).  Returns figures of the run."""
    n_cu = engine.device_info()["n_cu"]
    assert n_cu >= 1
    n = 48 * n_cu + 37
    waves = 4 * 8 * n_cu
    fig = dict(n_cu=n_cu, reads=n, items=2 * n, launched_waves=waves, within=[])
    assert 2 * n > 3 * waves
    for c in many_reference(n_cu):
        m = len(c["unit"])
        assert len(c["reads"]) == n
        fwd, rc = _call(engine, c["unit"], c["reads"], c["k"])
        for got, want, strand in ((fwd, c["want"][0], "forward"), (rc, c["want"][1], "reverse complement")):
            bad = [i for i in range(n) if got[i] != want[i]]
            assert not bad, f"unit of {m} bases, {strand}: {len(bad)} of {n} reads differ from the oracle, first at read {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"
        border = 16 * n_cu
        assert 2 * border == waves
        fwd, rc = _call(engine, c["unit"], c["reads"][5:5 + border], c["k"])
        assert fwd == c["want"][0][5:5 + border] and rc == c["want"][1][5:5 + border], f"unit of {m} bases: one item per wave"
        fig["within"].append(c["within"])
    return fig


def cli_case(n_cu):
    """f.  (unit, [(name, read)], threshold, the bytes rr.py must write): 48 x n_cu + 37 short reads against a unit of 130 bases."""
    c = many_reference(n_cu)[-1]
    unit, reads = c["unit"], c["reads"][5:] + c["reads"][5:10]
    assert len(unit) == 130 and len(reads) == 48 * n_cu + 37 and max(map(len, reads)) <= 136
    named = [(b"r%d" % i, r) for i, r in enumerate(reads)]
    keep = rr.recruited(unit, reads, c["k"])
    assert 4 * sum(keep) >= len(reads) and 4 * (len(reads) - sum(keep)) >= len(reads)
    want = b"".join(b">" + name + b"\n" + r + b"\n" for (name, r), k in zip(named, keep) if k)
    return unit, named, c["k"], want


def write_cli_input(d, unit, named):
    """unit.fasta and reads.fasta in directory d (an empty read is a header without a sequence line); returns their paths."""
    up, rp = os.path.join(d, "unit.fasta"), os.path.join(d, "reads.fasta")
    with open(up, "wb") as f:
        f.write(b">unit\n" + unit + b"\n")
    with open(rp, "wb") as f:
        for name, r in named:
            f.write(b">" + name + b" len=%d\n" % len(r) + (r + b"\n" if r else b""))
    return up, rp

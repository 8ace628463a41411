"""Statements of what cf_edit.hip computes, the seeded inputs of its tests, and the polished trees of the assembly tests.

* ``nw``: global unit-cost edit distance by plain dynamic programming in numpy, a row at a time.
* ``fr``: the same distance by furthest-reaching points on diagonals, the kernel's algorithm, in Python on PADDED copies.
* ``hpc``: homopolymer compression.
* ``WRONG_RULES``: plausible misreadings of the three; tests/golden/make_golden_edit.py fails unless each one changes a
  recorded case, so the goldens (the reference's vendored edlib and its own polisher methods) tell them apart.
* ``single_cases`` / ``batch_case`` / ``big_cases``: the inputs, from seeds alone.  tests/golden/edit_cases.json holds their
  SHA-256 and the reference's answers.
"""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "edit_cases.json")
WRONG_RULES = ("n_matches_anything", "case_folding", "no_clamp_at_n", "hpc_resets_at_tile_borders")
HPC_TILE = 2048          # (the tile of the scan of cf_prims.hip, in 8-byte groups: 16 384 bytes; any tile shows the misreading)


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---------------------------------------------------------------- statements
def _eq_table(wrong):
    t = np.arange(256, dtype=np.int64)
    if wrong == "case_folding":
        t[ord("a"):ord("z") + 1] -= 32
    return t


def nw(a, b, wrong=None):
    """Edit distance of two byte strings: cur = min(prev + 1, prev_shifted + neq), then minimum.accumulate(cur - j) + j."""
    t = _eq_table(wrong)
    a = t[np.frombuffer(bytes(a), np.uint8)]
    b = t[np.frombuffer(bytes(b), np.uint8)]
    j = np.arange(b.size + 1, dtype=np.int64)
    prev = j.copy()
    for i in range(a.size):
        neq = (b != a[i]).astype(np.int64)
        if wrong == "n_matches_anything":
            neq[(b == ord("N")) | (a[i] == ord("N"))] = 0
        cur = np.empty_like(prev)
        cur[0] = i + 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + neq)
        prev = np.minimum.accumulate(cur - j) + j
    return int(prev[-1])


def fr(a, b, k=None, wrong=None, want_reach=False):
    """The kernel's statement: F_0[0] = ext(0, 0); F_s[c] = ext(min(max(F[c] + 1, F[c-1], F[c+1] + 1), n, m - c), c) over
    max(-s, -n) <= c <= min(s, m); the first s with F_s[m - n] >= n; -1 when that s exceeds k.  The strings lie in one buffer as
    the device copy does: b follows a directly, zeros follow b.  want_reach: also the largest F ever held.  Without the clamp at
    n a run walks on into the bytes behind a; the target diagonal is still clamped by m - c = n, and a value beyond n helps a
    neighbour no more than n does, so that misreading shows in the reach (rows that do not exist), never in the distance."""
    a, b = bytes(a), bytes(b)
    n, m = len(a), len(b)
    pa, pb = a + b + bytes(64 + m), b + bytes(64 + n + m)
    k = max(n, m) if k is None else min(k, max(n, m))

    def top(c):
        return m - c if wrong == "no_clamp_at_n" else min(n, m - c)

    def ext(i, c):
        while i < top(c) and pa[i] == pb[i + c]:
            i += 1
        return i
    f = {0: ext(0, 0)}
    s, reach = 0, f[0]
    while not (f.get(m - n, -1) >= n):
        if s == k:
            s = -1
            break
        s += 1
        g = {}
        for c in range(max(-s, -n), min(s, m) + 1):
            v = max(f.get(c, -10 ** 9) + 1, f.get(c - 1, -10 ** 9), f.get(c + 1, -10 ** 9) + 1)
            g[c] = ext(min(v, top(c)), c)
        f = g
        reach = max(reach, max(f.values()))
    return (s, reach) if want_reach else s


def hpc(s, wrong=None):
    """Keep byte i iff i == 0 or s[i] != s[i - 1]."""
    s = np.frombuffer(bytes(s), np.uint8)
    if s.size == 0:
        return b""
    keep = np.ones(s.size, bool)
    keep[1:] = s[1:] != s[:-1]
    if wrong == "hpc_resets_at_tile_borders":
        keep[::HPC_TILE * 8] = True
    return s[keep].tobytes()


# ---------------------------------------------------------------- inputs
def rand_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def mutate(rng, s, n_edits, alphabet=b"ACGT"):
    """n_edits substitutions, insertions and deletions at random places."""
    s = bytearray(s)
    for _ in range(n_edits):
        kind = int(rng.integers(0, 3))
        c = alphabet[int(rng.integers(0, len(alphabet)))]
        if kind == 0 and s:
            p = int(rng.integers(0, len(s)))
            s[p] = c if s[p] != c else alphabet[(alphabet.index(c) + 1) % len(alphabet)]
        elif kind == 1 or not s:
            s.insert(int(rng.integers(0, len(s) + 1)), c)
        else:
            del s[int(rng.integers(0, len(s)))]
    return bytes(s)


def hor_array(rng, unit_len, n_units=12, div=0.01):
    """n_units diverged copies of one random unit, and where each begins."""
    base = rand_seq(rng, unit_len)
    units = []
    for _ in range(n_units):
        u = bytearray(base)
        for p in rng.choice(unit_len, max(1, int(unit_len * div)), replace=False):
            u[p] = b"ACGT"[(b"ACGT".index(u[p]) + 1 + int(rng.integers(0, 3))) % 4]
        units.append(bytes(u))
    return units


LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65)
IDENT_LEN = 100000


def ident_positions(lane_bytes, turn_bytes):
    """A mismatch at byte 0, at the last byte, and on either side of every border of the cooperative extension: the lane's own
    bytes, the wave's 16-byte pieces, its 1 KB chunks and its turns — counted from the start and from behind a mismatch."""
    pos = {0, IDENT_LEN - 1}
    for border in (lane_bytes, 16, 1024, turn_bytes, 2 * turn_bytes, lane_bytes + turn_bytes, lane_bytes + 1024):
        pos.update((border - 1, border, border + 1))
    return sorted(pos)


def single_cases(lane_bytes=32, turn_bytes=4096, small_only=False):
    """[(name, a, b)]: every case that is one pair.  small_only: those with d^2 <= 10^6 (the emulator's share)."""
    out = []
    rng = np.random.default_rng(20260001)
    for la in LENGTHS:
        for lb in LENGTHS:
            a = rand_seq(rng, la)
            b = mutate(rng, a, 2)[:lb] if (la + lb) % 3 == 0 else rand_seq(rng, lb)
            b = b + rand_seq(rng, lb - len(b))
            out.append((f"len_{la}_{lb}", a, b))
    out.append(("N_and_case", b"ACGTNNACGTacgtNACGT", b"ACGTACACGTACGTNNCGT"))
    out.append(("empty_empty", b"", b""))
    base = rand_seq(rng, IDENT_LEN)
    out.append(("ident", base, base))
    for p in ident_positions(lane_bytes, turn_bytes):
        b = bytearray(base)
        b[p] = ord("A") if b[p] != ord("A") else ord("C")
        out.append((f"ident_mismatch_{p}", base, bytes(b)))
    b = bytearray(base)
    for p in (lane_bytes + 5, lane_bytes + 5 + turn_bytes, 50000):
        b[p] = ord("A") if b[p] != ord("A") else ord("C")
    out.append(("ident_three_mismatches", base, bytes(b[:50100] + b[50101:])))
    for unit_len in (171, 2055):
        units = hor_array(rng, unit_len)
        a = b"".join(units)
        if small_only and unit_len * unit_len > 10 ** 6:
            continue
        out.append((f"hor{unit_len}_unit_deleted", a, b"".join(units[:5] + units[6:])))
        out.append((f"hor{unit_len}_unit_inserted", a, b"".join(units[:5] + [units[5]] + units[5:])))
    out.append(("related_1200", *(lambda s: (s, mutate(rng, s, 40)))(rand_seq(rng, 1200))))
    out.append(("unrelated_600", rand_seq(rng, 600), rand_seq(rng, 640)))
    return out


def offset_cases():
    """[(name, data, a_off, b_off, a, b)]: one related pair at every pair of start offsets mod 8."""
    rng = np.random.default_rng(20260002)
    out = []
    for oa in range(8):
        for ob in range(8):
            a = rand_seq(rng, 90 + oa)
            b = mutate(rng, a, 3)
            fill = (ob - (oa + len(a))) % 8
            data = rand_seq(rng, oa) + a + rand_seq(rng, fill) + b
            sb = oa + len(a) + fill
            assert sb % 8 == ob
            out.append((f"off_{oa}_{ob}", data, [oa, oa + len(a)], [sb, sb + len(b)], a, b))
    return out


def switch_cases(lds_diags):
    """Two unrelated pairs whose band (length + 1 diagonals for equal even lengths and no limit) is just below and just above the
    switch point between wavefronts in LDS and in HBM."""
    rng = np.random.default_rng(20260003)
    lo = (lds_diags - 2) & ~1
    hi = (lds_diags + 2) & ~1
    return [(f"switch_below_{lo}", rand_seq(rng, lo), rand_seq(rng, lo)), (f"switch_above_{hi}", rand_seq(rng, hi), rand_seq(rng, hi))]


def big_cases():
    """The cases of hardware size only."""
    rng = np.random.default_rng(20260004)
    return [("unrelated_20000", rand_seq(rng, 20000), rand_seq(rng, 20000))]


BATCH_PAIRS = 3000


def batch_case(n_pairs=BATCH_PAIRS):
    """(data, a_off, b_off): n_pairs related pairs of 150 .. 2 100 bytes in shuffled size order, the a strings back to back in front
    of the b strings; some pairs identical, some with an N or a lower-case letter."""
    rng = np.random.default_rng(20260005)
    aa, bb = [], []
    for p in range(n_pairs):
        a = bytearray(rand_seq(rng, int(rng.integers(150, 2101))))
        if p % 7 == 0:
            a[int(rng.integers(0, len(a)))] = ord("N")
        if p % 11 == 0:
            q = int(rng.integers(0, len(a)))
            a[q] = a[q] | 0x20
        b = mutate(rng, bytes(a), int(rng.integers(0, 9)))
        if p % 13 == 0:
            b = b.replace(b"N", b"A").upper()
        aa.append(bytes(a))
        bb.append(b)
    a_off = np.zeros(n_pairs + 1, np.int64)
    np.cumsum([len(s) for s in aa], out=a_off[1:])
    b_off = np.zeros(n_pairs + 1, np.int64)
    np.cumsum([len(s) for s in bb], out=b_off[1:])
    return b"".join(aa) + b"".join(bb), a_off, b_off + a_off[-1]


def hpc_case(long_runs=True):
    """(data, off): sequences with runs longer than a scan tile, runs that span the border of two sequences, empty sequences."""
    rng = np.random.default_rng(20260006)
    seqs = [b"", rand_seq(rng, 5), b"A" * 3, b"A" * 4 + b"C", b"", b"", b"C" * 9 + rand_seq(rng, 100, b"AACCCGT"), b"T"]
    seqs.append(rand_seq(rng, 3000, b"AAACGGT") + b"G" * (40000 if long_runs else 70) + b"GT" + b"T" * 17)
    seqs.append(b"T" * 8 + rand_seq(rng, 777))
    seqs.append(b"")
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return b"".join(seqs), off, seqs


# ---------------------------------------------------------------- polished trees
TREES = (
    dict(name="tiny_plain", fixture="tiny", num_iters=4, multiline=0, gap=False, seed=11),
    dict(name="lowcov_multiline", fixture="lowcov", num_iters=3, multiline=60, gap=False, seed=12),
    dict(name="tiny_gap", fixture="tiny", num_iters=2, multiline=0, gap=True, seed=13),
)


def placement_csv(fixture, wd):
    with open(os.path.join(ROOT, "tests", "golden", f"{fixture}.json")) as f:
        g = json.load(f)
    path = os.path.join(wd, f"{fixture}.read_positions.csv")
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in g["read_positions"]["placed"] + g["read_positions"]["none"]))
    return path


def fabricate_tree(spec, outdir):
    """Writes pos_P/polished_i.fasta into an exported tree: the position's median read unit with seeded edits that shrink per
    iteration (iteration i is the unit with max(0, 7 - 2 i) .. edits; the last iterations are nearly equal).  A gap tree loses
    a whole position directory in the middle.  Returns {relative file name: sha256}."""
    rng = np.random.default_rng(spec["seed"])
    positions = sorted(int(d[4:]) for d in os.listdir(outdir) if d.startswith("pos_"))
    made = {}
    for pos in positions:
        d = os.path.join(outdir, f"pos_{pos}")
        with open(os.path.join(d, "median_read_unit.fasta")) as f:
            unit = "".join(ln.strip() for ln in f.read().splitlines()[1:]).encode()
        for i in range(1, spec["num_iters"] + 1):
            seq = mutate(rng, unit, max(0, 7 - 2 * i) + (1 if (pos + i) % 5 == 0 else 0)).decode()
            w = spec["multiline"]
            body = "\n".join(seq[j:j + w] for j in range(0, len(seq), w)) if w else seq
            text = f">contig_1 polished {i}\n{body}\n" + (">contig_2\nACGT\n" if pos % 3 == 0 else "")
            with open(os.path.join(d, f"polished_{i}.fasta"), "w") as f:
                f.write(text)
            made[f"pos_{pos}/polished_{i}.fasta"] = sha(text.encode())
    return made


def gap_position(outdir):
    positions = sorted(int(d[4:]) for d in os.listdir(outdir) if d.startswith("pos_"))
    return positions[len(positions) // 2]


# ---------------------------------------------------------------- shared checks (emulator and hardware)
def one_pair(engine, a, b, k=2 ** 31 - 1):
    d, ms = engine.edit_distances(a + b, [0, len(a)], [len(a), len(a) + len(b)], k)
    assert ms >= 0.0
    return int(d[0])


def check_singles(engine, golden, cases):
    """Every case as a launch of its own and all of them as one batch, against the reference's recorded distances."""
    for name, a, b in cases:
        g = golden["single"][name]
        assert (sha(a), sha(b)) == (g["sha_a"], g["sha_b"]), f"{name}: the generated input is not the recorded one"
        assert one_pair(engine, a, b) == g["distance"], name
    aa = b"".join(a for _, a, _ in cases)
    bb = b"".join(b for _, _, b in cases)
    a_off = np.cumsum([0] + [len(a) for _, a, _ in cases])
    b_off = np.cumsum([0] + [len(b) for _, _, b in cases]) + len(aa)
    d, _ = engine.edit_distances(aa + bb, a_off, b_off)
    assert d.tolist() == [golden["single"][name]["distance"] for name, _, _ in cases]


def check_limits(engine, golden, cases):
    """k equal to the distance gives the distance, k - 1 gives -1, k = 0 tells equal from different."""
    for name, a, b in cases:
        w = golden["single"][name]["distance"]
        assert one_pair(engine, a, b, w) == w, name
        if w > 0:
            assert one_pair(engine, a, b, w - 1) == -1, name
        assert one_pair(engine, a, b, 0) == (0 if w == 0 else -1), name


def build_tree(spec, report_fn, wd):
    """The exported tree of a fixture with its fabricated polished_i.fasta: (params of the assembly, {file: sha256})."""
    import math
    import types
    from centroflye_amd import eltr_polisher
    unit = os.path.join(wd, "unit.fasta")
    with open(unit, "w") as f:
        f.write(">u\nACGT\n")
    outdir = os.path.join(wd, spec["name"])
    params = types.SimpleNamespace(unit=unit, ncrf=report_fn, outdir=outdir, read_placement=placement_csv(spec["fixture"], wd), min_pos=0,
                                   max_pos=math.inf, num_iters=spec["num_iters"])
    pol = eltr_polisher.ELTR_Polisher(params)
    files = pol.export_read_units(pol.map_pos2read())
    return pol, files, fabricate_tree(spec, outdir)


def digest_finals(outdir):
    res = {}
    for fn in sorted(os.listdir(outdir)):
        if fn.startswith("final_sequence"):
            with open(os.path.join(outdir, fn), "rb") as f:
                res[fn] = sha(f.read())
    return res

"""The rule of the built-in monomer decomposer (include/cfhip.h at cf_monodec_run) restated in plain Python, cell by
cell (`decompose`), and a second time a row at a time in numpy (`decompose_np`: moves and boundary entries instead of the cells, the
way the device keeps them), which equals the plain one on every small case and serves the larger shapes.  There is no reference
function behind the decomposer; what pins the restatement is in tests/test_emu_monodec.py: the literal cases below, the planted
misreadings (WRONG_RULES) that each change a literal, and the plain Needleman-Wunsch score against every sequence of monomers.
The checks of the device against the restatement that the emulator suite and the GPU suite share are here too."""
import itertools

import numpy as np

DEFAULT = (1, 1, 1)
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return bytes(s).translate(_RC)[::-1]


def _upper(b):
    return b - 32 if 97 <= b <= 122 else b


# ---------------------------------------------------------------- the plain restatement
WRONG_RULES = ("no feedback term", "(b) before (a)", "ties to the larger k", "ties to '-'", "case-sensitive comparison",
               "E[i] without E[i-1] - G", "a horizontal that crosses a monomer start")


def _fill(us, r, scores, wrong):
    """E[i] and V[i][k][j] of one strand's problem."""
    M, X, G = scores
    n = len(r)
    E = [0] * (n + 1)
    V = [[[-(j + 1) * G for j in range(len(u))] for u in us]]
    for i in range(1, n + 1):
        x = r[i - 1] if wrong == "case-sensitive comparison" else _upper(r[i - 1])
        A = []
        for k, u in enumerate(us):
            row = []
            for j in range(len(u)):
                d = (E[i - 1] if j == 0 else V[i - 1][k][j - 1]) + (M if x == u[j] else -X)
                row.append(max(d, V[i - 1][k][j] - G))
            A.append(row)
        Vp = [[max(A[k][j - t] - t * G for t in range(j + 1)) for j in range(len(u))] for k, u in enumerate(us)]
        e = max(Vp[k][len(u) - 1] for k, u in enumerate(us))
        if wrong != "E[i] without E[i-1] - G":
            e = max(e, E[i - 1] - G)
        E[i] = e
        if wrong == "no feedback term":
            V.append(Vp)
        else:
            V.append([[max(Vp[k][j], e - (j + 1) * G) for j in range(len(u))] for k, u in enumerate(us)])
    return E, V


def _walk(us, r, scores, E, V, wrong):
    """The walk from boundary n: (prefix, [(k, st, en, ops)]), instances left to right, ops left to right: M match, X mismatch,
    I a read base against nothing (rule b), D a monomer base against nothing (rule c)."""
    M, X, G = scores
    n = len(r)
    inst = []
    i = n
    prefix = 0
    steps = 0
    while i > 0:
        ks = [k for k, u in enumerate(us) if V[i][k][len(u) - 1] == E[i]]
        if not ks:
            prefix += 1
            i -= 1
            continue
        assert prefix == 0, "unassigned bases behind an instance"
        k = max(ks) if wrong == "ties to the larger k" else min(ks)
        u = us[k]
        j = len(u) - 1
        en = i - 1
        ops = []
        while j >= 0:
            steps += 1
            assert steps <= 4 * (n + sum(len(x) for x in us)) * (M + 1) + 16, "the walk does not end"
            v = V[i][k][j]
            a = b = False
            if i >= 1:
                x = r[i - 1] if wrong == "case-sensitive comparison" else _upper(r[i - 1])
                d = (E[i - 1] if j == 0 else V[i - 1][k][j - 1]) + (M if x == u[j] else -X)
                a = d == v
                b = V[i - 1][k][j] - G == v
            if wrong == "(b) before (a)" and b:
                a = False
            if a:
                ops.append("M" if x == u[j] else "X")
                i -= 1
                j -= 1
            elif b:
                ops.append("I")
                i -= 1
            else:
                ops.append("D")
                j -= 1
                if j < 0 and k > 0 and wrong == "a horizontal that crosses a monomer start":
                    # (the misreading: from a monomer's first column on into the last column of the monomer in front of it)
                    inst.append((k, i, en, "".join(reversed(ops))))
                    k -= 1
                    u = us[k]
                    j, en, ops = len(u) - 1, i - 1, []
        inst.append((k, i, en, "".join(reversed(ops))))
    return prefix, inst[::-1]


def decompose(monos, r, scores=DEFAULT, wrong=None):
    """{strand, score, prefix, inst: [(k, st, en, ops)]} of one read; n = 0: no instances, score 0, strand 0."""
    monos = [bytes(m) for m in monos]
    r = bytes(r)
    res = []
    for us in (monos, [rc(m) for m in monos]):
        E, V = _fill(us, r, scores, wrong)
        res.append((E, V, us))
    s = 1 if res[1][0][-1] > res[0][0][-1] else 0
    if wrong == "ties to '-'":
        s = 1 if res[1][0][-1] >= res[0][0][-1] else 0
    if not r:
        s = 0
    E, V, us = res[s]
    prefix, inst = _walk(us, r, scores, E, V, wrong)
    return dict(strand=s, score=E[-1], prefix=prefix, inst=inst)


# ---------------------------------------------------------------- a row at a time
def _solve_np(us, r, scores, moves):
    """E[n] of one strand; with moves also the move of every cell (1, 2, 3 = rules a, b, c) and the boundary entries."""
    M, X, G = scores
    n = len(r)
    lens = np.array([len(u) for u in us], np.int64)
    L = int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)])
    u = np.frombuffer(b"".join(us), np.uint8)
    jj = np.concatenate([np.arange(x, dtype=np.int64) for x in lens])
    seg = np.repeat(np.arange(len(us), dtype=np.int64), lens)
    starts, ends = off[:-1], off[1:] - 1
    big = np.int64(1) << 40
    V = -(jj + 1) * G
    e_prev = 0
    rr = np.frombuffer(bytes(r).upper(), np.uint8)
    mv = np.zeros((n, L), np.uint8) if moves else None
    kstar = np.full(n + 1, -1, np.int64)
    for i in range(1, n + 1):
        w = np.where(u == rr[i - 1], M, -X).astype(np.int64)
        din = np.empty(L, np.int64)
        din[1:] = V[:-1]
        din[starts] = e_prev
        D = din + w
        up = V - G
        A = np.maximum(D, up)
        Vp = np.maximum.accumulate(A + jj * G + seg * big) - jj * G - seg * big
        best = Vp[ends]
        e = max(int(best.max()), e_prev - G)
        Vn = np.maximum(Vp, e - (jj + 1) * G)
        if moves:
            mv[i - 1] = np.where(D == Vn, 1, np.where(up == Vn, 2, 3))
            hit = np.nonzero(best == e)[0]
            kstar[i] = hit[0] if hit.size else -1
        V = Vn
        e_prev = e
    return e_prev, mv, kstar


def decompose_np(monos, r, scores=DEFAULT):
    monos = [bytes(m) for m in monos]
    r = bytes(r)
    n = len(r)
    if n == 0:
        return dict(strand=0, score=0, prefix=0, inst=[])
    both = [monos, [rc(m) for m in monos]]
    sc = [_solve_np(us, r, scores, False)[0] for us in both]
    s = 1 if sc[1] > sc[0] else 0
    us = both[s]
    _, mv, kstar = _solve_np(us, r, scores, True)
    off = np.concatenate([[0], np.cumsum([len(u) for u in us])])
    ru = bytes(r).upper()
    inst = []
    i, prefix = n, 0
    while i > 0:
        k = int(kstar[i])
        if k < 0:
            prefix = i
            break
        j, en, ops = len(us[k]) - 1, i - 1, []
        while j >= 0:
            m = 3 if i == 0 else int(mv[i - 1, off[k] + j])
            if m == 1:
                ops.append("M" if ru[i - 1] == us[k][j] else "X")
                i -= 1
                j -= 1
            elif m == 2:
                ops.append("I")
                i -= 1
            else:
                ops.append("D")
                j -= 1
        inst.append((k, i, en, "".join(reversed(ops))))
    return dict(strand=s, score=sc[s], prefix=prefix, inst=inst[::-1])


# ---------------------------------------------------------------- invariants, the independent check
def score_of(res, scores):
    M, X, G = scores
    ops = "".join(o for _, _, _, o in res["inst"])
    return M * ops.count("M") - X * ops.count("X") - G * (ops.count("I") + ops.count("D")) - G * res["prefix"]


def check_invariants(monos, r, scores, res):
    """the instances tile [prefix, n), each covers its whole monomer and at least one read base, and the ops add up to the score"""
    n = len(r)
    if n == 0:
        assert res == dict(strand=0, score=0, prefix=0, inst=[])
        return
    pos = res["prefix"]
    for k, st, en, ops in res["inst"]:
        assert st == pos and st <= en, (st, en, pos)
        assert ops.count("M") + ops.count("X") + ops.count("D") == len(monos[k])
        assert ops.count("M") + ops.count("X") + ops.count("I") == en - st + 1
        pos = en + 1
    assert pos == n
    assert score_of(res, scores) == res["score"]


def nw_score(a, b, scores):
    """plain global Needleman-Wunsch of the read a against the sequence b, linear gaps"""
    M, X, G = scores
    prev = [-j * G for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        cur = [-i * G] + [0] * len(b)
        x = _upper(a[i - 1])
        for j in range(1, len(b) + 1):
            cur[j] = max(prev[j - 1] + (M if x == b[j - 1] else -X), prev[j] - G, cur[j - 1] - G)
        prev = cur
    return prev[len(b)]


def brute_score(monos, r, scores):
    """the best NW score of the read against the concatenation of ANY sequence of 0 .. n monomers of one strand, both strands"""
    best = None
    for us in (monos, [rc(m) for m in monos]):
        for cnt in range(len(r) + 1):
            for seq in itertools.product(range(len(us)), repeat=cnt):
                s = nw_score(r, b"".join(us[k] for k in seq), scores)
                best = s if best is None or s > best else best
    return best


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n)) if n else b""


def small_cases(n_cases=240, seed=2027):
    """seeded small cases: K <= 3 monomers of <= 4 bases, reads of <= 6 bytes over a small alphabet so that ties are common"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_cases):
        alpha = (b"AC", b"ACG", b"ACGT")[c % 3]
        monos = [rand_seq(rng, int(rng.integers(1, 5)), alpha) for _ in range(int(rng.integers(1, 4)))]
        r = rand_seq(rng, int(rng.integers(0, 7)), alpha + (b"Na" if c % 5 == 0 else b""))
        scores = [(1, 1, 1), (2, 3, 1), (1, 1, 2), (3, 1, 2), (1, 2, 3)][c % 5]
        out.append((monos, r, scores))
    return out


# ---------------------------------------------------------------- the literal cases: (name, monomers, read, scores, want)
LITERALS = []   # filled below
LITERAL_SHOWS = {}


def _lit(name, shows, monos, r, scores, want):
    LITERALS.append((name, monos, r, scores, want))
    LITERAL_SHOWS[name] = shows


_lit("one monomer twice", "K = 1", [b"ACGT"], b"ACGTACGT", DEFAULT,
     dict(strand=0, score=8, prefix=0, inst=[(0, 0, 3, "MMMM"), (0, 4, 7, "MMMM")]))
_lit("a monomer of one base", "a monomer of length 1", [b"A", b"CG"], b"ACGA", DEFAULT,
     dict(strand=0, score=4, prefix=0, inst=[(0, 0, 0, "M"), (1, 1, 2, "MM"), (0, 3, 3, "M")]))
_lit("deleted first bases", "an instance with deleted first bases, through the feedback", [b"ACGTACGT"], b"ACGTACGTCGTACGT", (2, 3, 1),
     dict(strand=0, score=29, prefix=0, inst=[(0, 0, 7, "MMMMMMMM"), (0, 8, 14, "DMMMMMMM")]))
_lit("deleted first bases of the second monomer", "the horizontal out of a first column ends at the boundary", [b"GGGG", b"ACGTACGT"],
     b"ACGTACGTCGTACGT", (2, 3, 1), dict(strand=0, score=29, prefix=0, inst=[(1, 0, 7, "MMMMMMMM"), (1, 8, 14, "DMMMMMMM")]))
_lit("deleted tail", "an instance with a deleted tail", [b"ACGTACGT"], b"ACGTACACGTACGT", (2, 3, 1),
     dict(strand=0, score=26, prefix=0, inst=[(0, 0, 5, "MMMMMMDD"), (0, 6, 13, "MMMMMMMM")]))
_lit("inserted run", "an inserted run", [b"ACGTTGCA"], b"ACGTGGTGCA", (2, 3, 1),
     dict(strand=0, score=14, prefix=0, inst=[(0, 0, 9, "MMMMIIMMMM")]))
_lit("leading prefix", "a leading prefix", [b"ACGTACGT"], b"TTACGTACGT", (1, 3, 1),
     dict(strand=0, score=6, prefix=2, inst=[(0, 2, 9, "MMMMMMMM")]))
_lit("two equal monomers", "a tie between two monomers going to the smaller k", [b"ACG", b"ACG", b"TTT"], b"ACGTTTACG", DEFAULT,
     dict(strand=0, score=9, prefix=0, inst=[(0, 0, 2, "MMM"), (2, 3, 5, "MMM"), (0, 6, 8, "MMM")]))
_lit("palindrome", "a '+' / '-' tie going to '+'", [b"ACGT"], b"ACGTACGT", (2, 1, 1),
     dict(strand=0, score=16, prefix=0, inst=[(0, 0, 3, "MMMM"), (0, 4, 7, "MMMM")]))
_lit("reverse strand", "a '-' winner", [b"AACC", b"GGGT"], b"ACCCGGTT", DEFAULT,
     dict(strand=1, score=8, prefix=0, inst=[(1, 0, 3, "MMMM"), (0, 4, 7, "MMMM")]))
_lit("N and lower case", "an N and a lower-case base", [b"ACGT"], b"AcNTacgt", DEFAULT,
     dict(strand=0, score=6, prefix=0, inst=[(0, 0, 3, "MMXM"), (0, 4, 7, "MMMM")]))
_lit("short read", "a read shorter than every monomer", [b"ACGTAC", b"GGTTAA"], b"GTT", DEFAULT,
     dict(strand=0, score=0, prefix=0, inst=[(1, 0, 2, "DMMMDD")]))
_lit("empty read", "n = 0", [b"ACGT"], b"", DEFAULT,
     dict(strand=0, score=0, prefix=0, inst=[]))
_lit("mismatch", "a mismatch inside an instance", [b"ACGTAC"], b"ACCTAC", (2, 1, 3),
     dict(strand=0, score=9, prefix=0, inst=[(0, 0, 5, "MMXMMM")]))
_lit("diagonal or vertical", "rule (a) before rule (b)", [b"AAC"], b"AAAC", DEFAULT,
     dict(strand=0, score=2, prefix=0, inst=[(0, 0, 0, "DMD"), (0, 1, 3, "MMM")]))
_lit("larger k alone", "the larger k where only it fits", [b"AAAA", b"CCCC"], b"CCCCAAAA", DEFAULT,
     dict(strand=0, score=8, prefix=0, inst=[(1, 0, 3, "MMMM"), (0, 4, 7, "MMMM")]))


def check_literal(name, monos, r, scores, want, decomposer=decompose):
    got = decomposer(monos, r, scores)
    check_invariants(monos, r, scores, got)
    return got == want


def killers():
    """for every planted misreading the literal cases whose result it changes (or whose walk it breaks)"""
    out = {}
    for wrong in WRONG_RULES:
        hit = []
        for name, monos, r, scores, want in LITERALS:
            try:
                got = decompose(monos, r, scores, wrong=wrong)
            except (AssertionError, IndexError, ValueError):
                got = None
            if got != want:
                hit.append(name)
        out[wrong] = hit
    return out


# ---------------------------------------------------------------- the report
def tsv_lines(names, mono_names, results, monos, min_identity=69):
    """the six columns of decomposition.tsv from the restatement's results (one per read, in input order)"""
    out = []
    for name, res in zip(names, results):
        for k, st, en, ops in res["inst"]:
            m, cols = ops.count("M"), len(ops)
            out.append("%s\t%s%s\t%d\t%d\t%s\t%s\n" % (name, mono_names[k], "'" if res["strand"] else "", st, en, "%.2f" % (100 * m / cols),
                                                    "+" if 100 * m >= min_identity * cols else "?"))
    return "".join(out)


# ---------------------------------------------------------------- device == restatement (shared by the emulator and the GPU suite)
def run_device(eng, monos, reads, scores=DEFAULT):
    flat = b"".join(reads)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return eng.monodec(monos, flat, off, *scores)


def tallies(res):
    return [(k, st, en, o.count("M"), o.count("X"), o.count("I"), o.count("D")) for k, st, en, o in res["inst"]]


def check(eng, monos, reads, scores=DEFAULT, decomposer=decompose_np, wants=None):
    """every field of every read and every instance of the device's answer equals the restatement's"""
    info, ptr, inst = run_device(eng, monos, reads, scores)
    assert len(info) == len(reads) and len(ptr) == len(reads) + 1 and ptr[0] == 0 and ptr[-1] == len(inst)
    wants = wants if wants is not None else [decomposer(monos, r, scores) for r in reads]
    for q, (r, want) in enumerate(zip(reads, wants)):
        got = tuple(int(x) for x in info[q])
        assert got == (1 if len(r) else 0, want["strand"], want["score"], len(want["inst"]), want["prefix"]), (q, got, want)
        assert [tuple(int(x) for x in row) for row in inst[ptr[q]:ptr[q + 1]]] == tallies(want), (q, want)
    return info, ptr, inst, wants


def monomers_with_lengths(rng, lens):
    return [rand_seq(rng, int(x)) for x in lens]


def noisy_read(rng, monos, n_mono, strand, err=0.06, start=None):
    """monomers in cyclic order from a random one, with substitutions, insertions and deletions at rate err in all; '-': its RC"""
    k = int(rng.integers(0, len(monos))) if start is None else start
    s = bytearray()
    for x in range(n_mono):
        s += monos[(k + x) % len(monos)]
    out = bytearray()
    for b in s:
        p = rng.random()
        if p < err / 3:
            continue
        if p < 2 * err / 3:
            out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            continue
        if p < err:
            out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
        out.append(b)
    out = bytes(out)
    return rc(out) if strand else out


def split_lengths(L, parts):
    """`parts` positive lengths that add up to L, the borders given by the caller's cut points"""
    cuts = [0] + sorted(parts) + [L]
    assert all(b > a for a, b in zip(cuts, cuts[1:])), cuts
    return [b - a for a, b in zip(cuts, cuts[1:])]


def noisy_stretch(rng, monos, n_bases, strand, err=0.06):
    """about n_bases of the monomers in cyclic order from a random one, cut inside a monomer, with errors; '-': its RC"""
    total = sum(len(m) for m in monos)
    r = noisy_read(rng, monos, (n_bases * len(monos)) // total + 2, strand, err)
    return r[:n_bases] if rng.random() < 0.5 else r[-n_bases:]


def check_columns(eng, L, cuts, n_reads=3, read_monos=3, seed=0, scores=(2, 3, 2), read_bases=None):
    """L columns cut into monomers at `cuts`; noisy reads of both strands in one call (read_bases: of about that many bases each)"""
    rng = np.random.default_rng(1000 * L + seed)
    monos = monomers_with_lengths(rng, split_lengths(L, cuts))
    if read_bases:
        reads = [noisy_stretch(rng, monos, read_bases + 7 * q, q & 1) for q in range(n_reads)]
    else:
        reads = [noisy_read(rng, monos, read_monos, q & 1) for q in range(n_reads)]
    reads.append(rand_seq(rng, 7))
    info, _, _, wants = check(eng, monos, reads, scores)
    return info, wants


# (L, cuts): monomer borders inside one thread's 16 columns, exactly on a thread border, one monomer over several threads
SMALL_COLUMNS = ((1, []), (2, [1]), (15, [7]), (16, []), (16, [3, 9]), (17, [16]), (63, [5, 16, 40]), (64, [32]), (65, [1, 64]),
                 (257, [100, 101, 256]), (257, []))


def check_row_chunks(eng, chunk=1024):
    """read lengths 0, 1 and around the chunk of read bytes staged in LDS"""
    rng = np.random.default_rng(43)
    monos = monomers_with_lengths(rng, [11, 17, 12])
    reads = [b"", rand_seq(rng, 1)] + [noisy_stretch(rng, monos, n, x & 1) for x, n in enumerate((chunk - 1, chunk, chunk + 1, 2 * chunk + 1))]
    reads.append(b"")
    info, ptr, inst, _ = check(eng, monos, reads)
    assert [int(x) for x in info["status"]] == [0, 1, 1, 1, 1, 1, 0] and ptr[1] == 0 and ptr[-1] == ptr[-2]


def check_literals(eng):
    for name, monos, r, scores, want in LITERALS:
        check(eng, monos, [r], scores, wants=[want])
    # all of one score set in one call
    group = [c for c in LITERALS if c[3] == DEFAULT and c[1] == [b"ACGT"]]
    assert len(group) >= 3
    check(eng, group[0][1], [c[2] for c in group], DEFAULT, wants=[c[4] for c in group])


def check_refusals(eng, DeviceError, max_cols=4096):
    import pytest
    rng = np.random.default_rng(5)
    monos = [b"ACGT", b"GGTA"]
    reads = [b"ACGTGGTAACGT", b"TACC"]
    base = check(eng, monos, reads)[:3]
    live = eng.stats()["hbm_bytes_live"]
    last = eng.monodec_info()
    flat, off = b"".join(reads), np.array([0, 12, 16], np.int64)

    def refused(match, *args, **kw):
        with pytest.raises(DeviceError, match=match) as e:
            eng.monodec(*args, **kw)
        assert "(-22)" in str(e.value)
        assert eng.stats()["hbm_bytes_live"] == live
        now = eng.monodec_info()
        assert {k: v for k, v in now.items() if k != "phase_ms"} == {k: v for k, v in last.items() if k != "phase_ms"}

    refused("no monomer", [], flat, off)
    refused("empty", [b"ACGT", b""], flat, off)
    refused("more than %d bases" % max_cols, [rand_seq(rng, max_cols - 3), b"ACGT"], flat, off)
    refused("not upper-case", [b"ACgT"], flat, off)
    refused("not upper-case", [b"ACNT"], flat, off)
    refused("at least 1", monos, flat, off, 0, 1, 1)
    refused("at least 1", monos, flat, off, 1, 0, 1)
    refused("at least 1", monos, flat, off, 1, 1, 0)
    refused("decrease", monos, flat, np.array([0, 12, 8], np.int64))
    refused("negative", monos, flat, np.array([-1, 12, 16], np.int64))
    # (n + L + 1) max(M, X, G) >= 2^31: n = 12, L = 8
    refused("2\\^31", monos, flat, off, 1, 1, (1 << 31) // 21 + 1)
    refused("2\\^31", monos, flat, off, (1 << 31) // 21 + 1, 1, 1)
    big = (1 << 31) // 21 - 1 if ((1 << 31) // 21) * 21 >= (1 << 31) else (1 << 31) // 21
    assert (12 + 8 + 1) * big < (1 << 31)
    check(eng, monos, reads, (1, big, 1))
    assert eng.stats()["hbm_bytes_live"] == live
    # the results of the run before a refusal are still there
    again = check(eng, monos, reads)[:3]
    refused("no monomer", [], flat, off)
    for a, b in zip(base, again):
        assert np.array_equal(a, b)


def check_saturating(eng):
    """gap costs near the int32 limit: (n + L + 1) max(M, X, G) just under 2^31"""
    rng = np.random.default_rng(23)
    monos = monomers_with_lengths(rng, [5, 33, 17, 1, 40])
    reads = [noisy_read(rng, monos, 4, q & 1, err=0.1) for q in range(3)]
    n = max(len(r) for r in reads)
    top = ((1 << 31) - 1) // (n + 96 + 1)
    for scores in ((1, 1, top), (top, 1, 1), (1, top, 1), (top, top, top), (top, 1, top // 2)):
        check(eng, monos, reads, scores)


def check_batches(eng, L=300):
    rng = np.random.default_rng(31)
    monos = monomers_with_lengths(rng, split_lengths(L, [50, 130, 131, 260]))
    reads = [noisy_read(rng, monos, 2 + q % 3, q & 1) for q in range(7)] + [b""]
    rw1 = (L + 15) // 16 + 1
    areas = sorted(len(r) * rw1 * 4 for r in reads if r)
    want = None
    for bb, n_batches in ((0, 1), (areas[-1] + areas[-2], None), (areas[0], 7), (100, 7)):
        with eng.knobs(monodec_batch_bytes=bb):
            info, ptr, inst, want = check(eng, monos, reads, wants=want)
            got = eng.monodec_info()
            assert got["n_move_pairs"] == 7 and got["n_score_pairs"] == 14 and got["n_reads"] == 8
            if n_batches:
                assert got["n_batches"] == n_batches, (bb, got)
            else:
                assert 1 < got["n_batches"] < 7


def check_more_pairs_than_the_launch_cap(eng):
    cap = eng.monodec_info()["launch_cap"]
    rng = np.random.default_rng(37)
    monos = monomers_with_lengths(rng, [7, 9, 4])
    n = cap // 2 + 9
    reads = [noisy_read(rng, monos, 1 + q % 4, q & 1, err=0.1) for q in range(n)]
    check(eng, monos, reads)
    assert eng.monodec_info()["n_score_pairs"] == 2 * sum(1 for r in reads if r) > cap


def check_hygiene(eng):
    rng = np.random.default_rng(41)
    monos = monomers_with_lengths(rng, [20, 31, 16])
    reads = [noisy_read(rng, monos, 5, q & 1) for q in range(4)]
    a = check(eng, monos, reads)
    live = eng.stats()["hbm_bytes_live"]
    b = check(eng, monos, reads, wants=a[3])
    assert eng.stats()["hbm_bytes_live"] == live
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    t0, s0 = eng.times(), {k: v for k, v in eng.stats().items()}
    check(eng, monos, reads, wants=a[3])
    assert eng.times() == t0 and eng.stats() == s0      # nothing is added to cf_times or cf_stats


# ---------------------------------------------------------------- D6Z1-shaped reads, the end-to-end check
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D6Z1_FASTA = os.path.join(GOLDEN, "D6Z1_monomers.fasta")
RATES = (0.02, 0.02, 0.015)      # substitutions, insertions, deletions per base: the generator's (tests/ualigncheck.py tandem_read)


def d6z1_monomers():
    """[(name, sequence)] of the 18 D6Z1 monomers (3 065 bases), names up to the first blank"""
    out, name, seq = [], None, []
    with open(D6Z1_FASTA, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(seq).upper()))
                name, seq = line[1:].split()[0], []
            else:
                seq.append(line.strip())
    out.append((name, b"".join(seq).upper()))
    return out


def hor_read(rng, seqs, ks, strand, rates=None):
    """The monomers ks in a row with errors at `rates` (None: error-free); '-': turned round.  Returns (bytes, origin): origin[i] =
    the index in ks of the monomer read base i came from (an inserted base belongs to the monomer in front of it)."""
    out, origin = bytearray(), []
    for x, k in enumerate(ks):
        for b in seqs[k]:
            if rates is not None:
                p = rng.random()
                if p < rates[2]:
                    continue
                if p < rates[2] + rates[0]:
                    b = int(rng.choice(np.frombuffer(b"ACGT".replace(bytes([b]), b""), np.uint8)))
                elif p < rates[2] + rates[0] + rates[1]:
                    out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
                    origin.append(x)
            out.append(b)
            origin.append(x)
    out = bytes(out)
    return (rc(out), origin[::-1]) if strand else (out, origin)


def hor_reads(n_reads, n_mono, seed, rates=None):
    """reads of n_mono D6Z1 monomers in HOR order from a random monomer on, one monomer of the row left out (the planted deletion);
    every other read is turned round.  [(name, bytes, planted ks, strand, origin)]"""
    rng = np.random.default_rng(seed)
    seqs = [s for _, s in d6z1_monomers()]
    out = []
    for q in range(n_reads):
        k0 = int(rng.integers(0, len(seqs)))
        ks = [(k0 + x) % len(seqs) for x in range(n_mono + 1)]
        del ks[int(rng.integers(1, n_mono))]
        r, origin = hor_read(rng, seqs, ks, q & 1, rates)
        out.append((b"hor_%s_%02d" % (b"noisy" if rates else b"clean", q), r, ks, q & 1, origin))
    return out


def planted_string(ks):
    return "".join(chr(65 + k) for k in ks)


def quality(reads, results):
    """(instances, those whose monomer is the planted one at the instance's middle base, those marked '?' at --min-identity 69)"""
    n = good = unsure = 0
    for (_, r, ks, strand, origin), res in zip(reads, results):
        for k, st, en, ops in res["inst"]:
            n += 1
            good += k == ks[origin[(st + en) // 2]]
            unsure += 100 * ops.count("M") < 69 * len(ops)
    return n, good, unsure


def write_fasta(path, reads):
    with open(path, "wb") as f:
        for name, seq in reads:
            f.write(b">" + name + b" a description\n" + seq + b"\n")


def check_cli_and_parser(tmp_path, monomers, reads, results, main, extra=()):
    """scripts/monomer_decomposer.py's main on the reads -> the TSV equals the restatement's byte for byte -> SD_Report reads it"""
    from centroflye_amd.sd_parser import SD_Report
    write_fasta(tmp_path / "reads.fasta", [(n, r) for n, r, *_ in reads])
    write_fasta(tmp_path / "monomers.fasta", monomers)
    out = tmp_path / "decomposition.tsv"
    assert main(["-s", str(tmp_path / "reads.fasta"), "-m", str(tmp_path / "monomers.fasta"), "-o", str(out), "-t", "7", *extra]) == 0
    assert sorted(os.listdir(tmp_path)) == ["decomposition.tsv", "monomers.fasta", "reads.fasta"]
    with open(out) as f:
        text = f.read()
    want = tsv_lines([n.decode() for n, *_ in reads], [n.decode() for n, _ in monomers], results, [s for _, s in monomers])
    assert text == want
    return SD_Report(str(out), str(tmp_path / "monomers.fasta"))

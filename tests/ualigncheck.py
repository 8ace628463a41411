"""The rule of the built-in tandem aligner (include/cfhip.h at cf_ualign_run) restated in plain Python, the literal cases
that pin the restatement, the planted misreadings they tell apart, the generators and the bodies of the tests that compare the
device (tests/test_gpu_ualign.py) or the host emulator (tests/test_emu_ualign.py) with it, field by field and op by op."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (10, 35, 33)
MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
WRONG_RULES = ("no_diag_wrap", "no_horiz_wrap", "b_before_a", "last_row", "last_col", "minus_first", "case_sensitive")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(u):
    return bytes(u).translate(_COMP)[::-1]


def upper(x):
    return x - 32 if 97 <= x <= 122 else x


# ---------------------------------------------------------------- the rule, cell by cell
def fill(u, r, scores=DEFAULT, wrong=()):
    """S[i][j], i = 0 .. n, j = 0 .. m - 1, as lists of ints."""
    M, X, G = scores
    m = len(u)
    S = [[0] * m]
    for i in range(1, len(r) + 1):
        prev, x = S[-1], r[i - 1]
        xu = x if "case_sensitive" in wrong else upper(x)
        A = []
        for j in range(m):
            diag_from = 0 if (j == 0 and "no_diag_wrap" in wrong) else prev[(j - 1) % m]
            A.append(max(0, diag_from + (M if xu == u[j] else -X), prev[j] - G))
        row = []
        for j in range(m):
            best = A[j]
            for t in range(1, m):
                if "no_horiz_wrap" in wrong and t > j:
                    break
                best = max(best, A[(j - t) % m] - t * G)
            row.append(best)
        S.append(row)
    return S


def end_cell(S, wrong=()):
    """(value, i, j) of the largest cell; the smallest i, then the smallest j among equals."""
    best = (0, 0, 0)
    for i, row in enumerate(S):
        for j, v in enumerate(row):
            if v > best[0] or (v == best[0] and v > 0 and (("last_row" in wrong and i > best[1]) or ("last_col" in wrong and i == best[1] and j > best[2]))):
                best = (v, i, j)
    return best


def walk(S, u, r, i, j, scores=DEFAULT, wrong=()):
    """(r_st, u_st, ops in read order) of the walk back from (i, j)."""
    M, X, G = scores
    m = len(u)
    ops, u_st = [], 0
    while S[i][j] != 0:
        x = r[i - 1]
        xu = x if "case_sensitive" in wrong else upper(x)
        diag_from = 0 if (j == 0 and "no_diag_wrap" in wrong) else S[i - 1][(j - 1) % m]
        a = diag_from + (M if xu == u[j] else -X) == S[i][j]
        b = S[i - 1][j] - G == S[i][j]
        if a and not (b and "b_before_a" in wrong):
            ops.append(MATCH if xu == u[j] else MISMATCH)
            u_st = j
            i, j = i - 1, (j - 1) % m
        elif b:
            ops.append(INS)
            i -= 1
        else:
            assert S[i][(j - 1) % m] - G == S[i][j], "the closed form makes rule (c) an equality"
            ops.append(DEL)
            u_st = j
            j = (j - 1) % m
    return i, u_st, ops[::-1]


def rows_of(u, r, r_st, u_st, ops):
    """(r_al, m_al): the two rows of the record; u is the strand's unit (RC(u) for '-')."""
    ra, ma, i, j = bytearray(), bytearray(), r_st, u_st
    for op in ops:
        if op != DEL:
            ra.append(r[i]); i += 1
        else:
            ra.append(45)
        if op != INS:
            ma.append(u[j % len(u)]); j += 1
        else:
            ma.append(45)
    return bytes(ra), bytes(ma)


def finish(u, r, strand, score, i, j, S, scores, wrong=()):
    us = rc(u) if strand else bytes(u)
    r_st, u_st, ops = walk(S, us, r, i, j, scores, wrong)
    r_al, m_al = rows_of(us, r, r_st, u_st, ops)
    cnt = [ops.count(k) for k in range(4)]
    return dict(strand=strand, score=score, r_st=r_st, r_en=i, u_st=u_st, m_al_len=cnt[0] + cnt[1] + cnt[3], ops=ops, counts=cnt, r_al=r_al, m_al=m_al)


def align(u, r, scores=DEFAULT, wrong=(), filler=fill):
    """None (no hit) or the record of read r against unit u: strand (0 '+', 1 '-'), score, r_st, r_en, u_st, m_al_len, ops, counts, r_al, m_al."""
    u, r = bytes(u), bytes(r)
    if not r:
        return None
    mats = [filler(u, r, scores, wrong), filler(rc(u), r, scores, wrong)]
    ends = [end_cell(S, wrong) for S in mats]
    strand = 1 if (ends[1][0] > ends[0][0] or ("minus_first" in wrong and ends[1][0] == ends[0][0])) else 0
    v, i, j = ends[strand]
    if v == 0:
        return None
    return finish(u, r, strand, v, i, j, mats[strand], scores, wrong)


# ---------------------------------------------------------------- the same, a row at a time in numpy (for the larger shapes)
def fill_np(u, r, scores=DEFAULT):
    """both strands at once: S[strand][i][j]"""
    M, X, G = scores
    m, n = len(u), len(r)
    dt = np.int32 if max(n * M + m * G, X + G) < 1 << 30 else np.int64
    us = np.stack([np.frombuffer(bytes(u), np.uint8), np.frombuffer(rc(u), np.uint8)])
    w_of = {b: np.where(us == upper(b), M, -X).astype(dt) for b in set(r)}
    S = np.zeros((2, n + 1, m), dt)
    jg = (np.arange(m, dtype=np.int64) * G).astype(dt)
    jg1 = jg + dt(G)
    d = np.empty((2, m), dt)
    for i in range(1, n + 1):
        prev = S[:, i - 1]
        d[:, 1:] = prev[:, :-1]
        d[:, 0] = prev[:, -1]
        d += w_of[r[i - 1]]
        np.maximum(d, prev - dt(G), out=d)
        np.maximum(d, 0, out=d)
        d += jg
        Sp = np.maximum.accumulate(d, axis=1)
        Sp -= jg
        np.maximum(Sp, Sp[:, -1:] - jg1, out=S[:, i])
    return S


def end_cell_np(S):
    v = int(S.max())
    if v == 0:
        return (0, 0, 0)
    i = int(np.argmax((S == v).any(axis=1)))
    return v, i, int(np.argmax(S[i] == v))


def align_np(u, r, scores=DEFAULT):
    u, r = bytes(u), bytes(r)
    if not r:
        return None
    mats = fill_np(u, r, scores)
    ends = [end_cell_np(S) for S in mats]
    strand = 1 if ends[1][0] > ends[0][0] else 0
    v, i, j = ends[strand]
    if v == 0:
        return None
    return finish(u, r, strand, v, i, j, mats[strand][:i + 1].tolist() if i * len(u) <= 1 << 16 else mats[strand], scores)


# ---------------------------------------------------------------- an independent check: plain Smith-Waterman against copies in a row
def sw_score(t, r, scores):
    """Best local score of r against the plain string t (linear gaps), and nothing else."""
    M, X, G = scores
    prev, best = [0] * (len(t) + 1), 0
    for x in r:
        xu, cur = upper(x), [0] * (len(t) + 1)
        for j in range(1, len(t) + 1):
            cur[j] = max(0, prev[j - 1] + (M if xu == t[j - 1] else -X), prev[j] - G, cur[j - 1] - G)
        best = max(best, max(cur))
        prev = cur
    return best


def copies(n, m, scores):
    M, _, G = scores
    return -(-(n * (G + M)) // (G * m)) + 2      # ceil(n (1 + M / G) / m) + 2


def score_of_ops(ops, scores):
    M, X, G = scores
    return sum((M, -X, -G, -G)[op] for op in ops)


# ---------------------------------------------------------------- the literal cases: name, unit, read, scores, expected
# expected: None, or (strand, score, r_st, r_en, u_st, r_al, m_al) with u_st the index in the strand's unit of the first column
LITERALS = []      # filled below
LITERAL_SHOWS = {}


def _lit(name, u, r, scores, want, shows):
    LITERALS.append((name, u, r, scores, want))
    LITERAL_SHOWS[name] = shows


_lit("two units on the diagonal", b"ACGT", b"ACGTACGT", DEFAULT, ("+", 80, 0, 8, 0, b"ACGTACGT", b"ACGTACGT"), "a diagonal from column m - 1 to column 0")
_lit("a deletion across the seam", b"ACGTTGCC", b"ACGTTGCGTTGCC", (2, 3, 1), ("+", 23, 0, 13, 0, b"ACGTTG---CGTTGCC", b"ACGTTGCCACGTTGCC"),
     "a horizontal from column 0 to column m - 1 (the deleted run C, C, A: 13 matches, 3 gap columns), a deleted run")
_lit("a unit of one base", b"A", b"CAAAC", DEFAULT, ("+", 30, 1, 4, 0, b"AAA", b"AAA"), "m = 1, flanks left out")
_lit("a read inside the unit", b"ACGTTGCC", b"GTTG", DEFAULT, ("+", 40, 0, 4, 2, b"GTTG", b"GTTG"), "a read shorter than the unit")
_lit("the other strand", b"AACCG", b"CGGTTCGGTT", DEFAULT, ("-", 100, 0, 10, 0, b"CGGTTCGGTT", b"CGGTTCGGTT"), "a '-' winner")
_lit("a palindromic unit", b"ACGT", b"ACGTAC", DEFAULT, ("+", 60, 0, 6, 0, b"ACGTAC", b"ACGTAC"), "an exact '+' / '-' tie")
_lit("the same hit twice", b"ACGT", b"ACGTNNACGT", DEFAULT, ("+", 40, 0, 4, 0, b"ACGT", b"ACGT"), "two end cells of equal score in different rows")
_lit("the same hit in two columns", b"ACTAC", b"AC", DEFAULT, ("+", 20, 0, 2, 0, b"AC", b"AC"), "two end cells of equal score in different columns of one row")
_lit("an inserted run", b"ACGTTGCC", b"ACGTTGCCACGTAATGCC", (5, 4, 3), ("+", 74, 0, 18, 0, b"ACGTTGCCACGTAATGCC", b"ACGTTGCCACGT--TGCC"), "an inserted run")
_lit("a deleted run", b"ACGTTGCC", b"ACGTTGCCACCCACGTTGCC", (5, 4, 3), ("+", 88, 0, 20, 0, b"ACGTTGCCAC----CCACGTTGCC", b"ACGTTGCCACGTTGCCACGTTGCC"),
     "a deleted run inside the unit")
_lit("soft-masked and N", b"ACGTTGCC", b"ACGTtgccACNTTGCC", DEFAULT, ("+", 115, 0, 16, 0, b"ACGTtgccACNTTGCC", b"ACGTTGCCACGTTGCC"), "an N and a lower-case stretch")
_lit("flanks", b"ACGTTGCC", b"GGGGGACGTTGCCACGTTGCCTTTTT", DEFAULT, ("+", 160, 5, 21, 0, b"ACGTTGCCACGTTGCC", b"ACGTTGCCACGTTGCC"), "flanks that are left out")
_lit("nothing of the unit", b"ACGT", b"NNNNNN", DEFAULT, None, "a read with no hit")
_lit("only other bytes", b"ACGT", b"acgu*-\x00\xff", (1, 1, 1), ("+", 3, 0, 3, 0, b"acg", b"ACG"), "lower case meets upper case, no other byte does")
_lit("a mismatch or an inserted byte", b"AA", b"ACA", (3, 1, 1), ("+", 5, 0, 3, 0, b"ACA", b"AAA"), "rule (a) before rule (b): 3 - 1 either way")
_lit("a deletion then a match", b"CA", b"CCA", (3, 1, 1), ("+", 8, 0, 3, 0, b"C-CA", b"CACA"), "a single deleted base")


def check_literal(name, u, r, scores, want, aligner=align, wrong=()):
    got = aligner(u, r, scores, wrong) if wrong else aligner(u, r, scores)
    if want is None or got is None:
        return got is None and want is None
    return ("+-"[got["strand"]], got["score"], got["r_st"], got["r_en"], got["u_st"], got["r_al"], got["m_al"]) == want


def killers():
    """misreading -> the literal cases it changes"""
    return {w: [c[0] for c in LITERALS if not check_literal(*c, wrong=(w,))] for w in WRONG_RULES}


# ---------------------------------------------------------------- generators
def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tolist())


def noisy(rng, t, p_del=0.02, p_sub=0.02, p_ins=0.015):
    out = bytearray()
    for b in t:
        x = rng.random()
        if x < p_del:
            continue
        if x < p_del + p_sub:
            out.append(rng.choice([c for c in b"ACGT" if c != b]))
        else:
            out.append(b)
        if rng.random() < p_ins:
            out.append(b"ACGT"[rng.integers(4)])
    return bytes(out)


def tandem_read(rng, u, n, strand=0, flank=0, rates=(0.02, 0.02, 0.015)):
    """About n bytes of the unit read cyclically from a random phase, with errors, between random flanks; '-' reads are turned round."""
    m = len(u)
    ph = int(rng.integers(m))
    body = noisy(rng, bytes(u[(ph + k) % m] for k in range(n)), *rates)
    if strand:
        body = rc(body)
    return rand_seq(rng, flank) + body + rand_seq(rng, flank)


def small_cases(seed=7, count=200):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(count):
        m = int(rng.integers(1, 13))
        u = rand_seq(rng, m)
        n = int(rng.integers(1, 61))
        scores = [DEFAULT, (2, 3, 1), (5, 4, 3), (1, 1, 1), (3, 1, 2)][c % 5]
        r = tandem_read(rng, u, n, strand=c % 3 == 2, flank=int(rng.integers(0, 4)), rates=(0.08, 0.08, 0.08))[:60]
        if r:
            out.append((u, r, scores))
    return out


# ---------------------------------------------------------------- device == restatement
def device(eng, u, reads, scores=DEFAULT):
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    hits, ptr, ops = eng.ualign_run(u, np.frombuffer(b"".join(reads), np.uint8), off, *scores)
    return hits, ptr, ops


def same(hit, ops, want):
    """the device's row of a read against the restatement's record, every field and every op"""
    if want is None:
        return all(int(hit[f]) == 0 for f in hit.dtype.names) and len(ops) == 0
    got = tuple(int(hit[f]) for f in hit.dtype.names)
    c = want["counts"]
    exp = (1, want["strand"], want["score"], want["r_st"], want["r_en"], want["u_st"], want["m_al_len"], len(want["ops"]), c[0], c[1], c[2], c[3])
    return got == exp and ops.tolist() == want["ops"]


def check(eng, u, reads, scores=DEFAULT, aligner=None, wants=None):
    """one call for all reads; returns the restatement's records"""
    aligner = aligner or (align if len(u) * max([len(r) for r in reads] + [0]) <= 4000 else align_np)
    wants = wants if wants is not None else [aligner(u, r, scores) for r in reads]
    hits, ptr, ops = device(eng, u, reads, scores)
    assert ptr.size == len(reads) + 1 and ptr[0] == 0 and ptr[-1] == ops.size
    for q, w in enumerate(wants):
        assert same(hits[q], ops[ptr[q]:ptr[q + 1]], w), (len(u), q, len(reads[q]), hits[q], w and {k: w[k] for k in w if k not in ("ops", "r_al", "m_al")})
    return wants


def check_literals(eng):
    for name, u, r, scores, want in LITERALS:
        got = check(eng, u, [r], scores, align)[0]
        assert (got is None) == (want is None), name
    # and the default-score cases of one unit in one call
    by_unit = {}
    for name, u, r, scores, want in LITERALS:
        if scores == DEFAULT:
            by_unit.setdefault(u, []).append(r)
    for u, reads in by_unit.items():
        check(eng, u, reads + [b""], DEFAULT, align)


UNIT_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 2055, 4095, 4096)


def unit_length_reads(rng, u, n_body, around_all):
    """reads of both strands, the lengths around the unit's (of every unit, or of the short ones), 0 and 1, only N"""
    m = len(u)
    reads = [tandem_read(rng, u, n_body, 0, 5), tandem_read(rng, u, n_body, 1, 5), b"", bytes(u[:1]), b"N" * 7]
    for n in (m - 1, m, m + 1):
        if n > 0 and (around_all or n <= 3 * n_body):
            body = tandem_read(rng, u, n + n // 20 + 8, int(rng.integers(2)))
            assert len(body) >= n
            reads.append(body[:n])
    return reads


def check_unit_lengths(eng, lengths, n_body, seed=11, around_all=False):
    info = eng.ualign_info()
    assert (info["cols_per_thread"], info["block"], info["max_unit"]) == (16, 256, 4096)
    # the borders: a thread's 16 columns, a wave's 64 x 16 = 1 024, the block's 256 x 16 = 4 096
    assert {15, 16, 17, 1024, 4095, 4096} <= set(UNIT_LENGTHS)
    rng = np.random.default_rng(seed)
    for m in lengths:
        u = rand_seq(rng, m)
        reads = unit_length_reads(rng, u, max(n_body, 2 * m if m <= 300 else 0), around_all)
        assert sorted({len(r) for r in reads[5:]}) == [n for n in (m - 1, m, m + 1) if n > 0] or (m > 300 and not around_all)
        wants = check(eng, u, reads)
        assert wants[0] is not None and wants[1] is not None or m < 4, m
        if m >= 15:
            assert wants[0]["strand"] == 0 and wants[1]["strand"] == 1, m      # both strands win inside one call


def check_too_long(eng, DeviceError):
    import pytest
    with pytest.raises(DeviceError, match="4097 bases"):
        eng.ualign_run(b"A" * 4097, np.frombuffer(b"ACGT", np.uint8), [0, 4])


def check_row_chunks(eng):
    """read lengths around the chunk in which the read goes through LDS"""
    chunk = eng.ualign_info()["row_chunk"]
    assert chunk == 1024
    rng = np.random.default_rng(3)
    u = rand_seq(rng, 37)
    reads = [tandem_read(rng, u, n, q & 1) for q, n in enumerate((chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1))]
    check(eng, u, reads, aligner=align_np)


def check_more_pairs_than_the_launch_cap(eng):
    cap = eng.ualign_info()["launch_cap"]
    rng = np.random.default_rng(5)
    u = rand_seq(rng, 9)
    reads = [tandem_read(rng, u, int(rng.integers(0, 30)), q % 3 == 0, int(rng.integers(0, 3))) for q in range(cap // 2 + cap + 3)]
    check(eng, u, reads, aligner=align_np)
    info = eng.ualign_info()
    assert info["n_score_pairs"] > cap and info["n_move_pairs"] > cap and info["n_reads"] == len(reads)


def check_batches(eng):
    """ualign_batch_bytes down to one pair per batch and below one pair's area"""
    rng = np.random.default_rng(9)
    u = rand_seq(rng, 40)      # 3 words per row
    reads = [tandem_read(rng, u, 100 + 10 * q, q & 1) for q in range(6)]
    wants = [align(u, r) for r in reads]
    areas = sorted(w["r_en"] * 3 * 4 for w in wants)
    default = eng.ualign_info()["batch_bytes"]
    assert 1 << 28 <= default <= 1 << 34
    for bytes_, n_batches in ((0, 1), (sum(areas), 1), (areas[-1] + areas[-2], None), (areas[-1], 6), (100, 6), (1, 6)):
        with eng.knobs(ualign_batch_bytes=bytes_):
            check(eng, u, reads, wants=wants)
            info = eng.ualign_info()
            assert info["batch_bytes"] == (bytes_ or default) and info["n_move_pairs"] == 6
            assert info["n_batches"] == n_batches or (n_batches is None and 1 < info["n_batches"] < 6), (bytes_, info)


def workload_pair(seed, m, n_body, flank=500):
    rng = np.random.default_rng(seed)
    u = rand_seq(rng, m)
    return u, tandem_read(rng, u, n_body, 0, flank)


def check_workload_pair(eng, m, n_body):
    u, r = workload_pair(2055, m, n_body)
    w = check(eng, u, [r], aligner=align_np)[0]
    # the array's ends: 500 random flank bases either side; a flank base continues the alignment only by chance
    assert w is not None and abs(w["r_st"] - 500) <= 20 and abs(w["r_en"] - (len(r) - 500)) <= 20
    ms = eng.ualign_info()["phase_ms"]
    assert ms["score"] > 0.0 and ms["moves"] > 0.0 and ms["total"] >= ms["score"] + ms["moves"]


def refusals(u=b"ACGT", reads=b"ACGTACGT"):
    r8 = np.frombuffer(reads, np.uint8)
    return [
        ("decreasing offsets", dict(unit=u, reads=r8, read_off=[0, 6, 4]), "decrease"),
        ("negative offset", dict(unit=u, reads=r8, read_off=[-1, 4]), "negative"),
        ("an empty unit", dict(unit=b"", reads=r8, read_off=[0, 8]), "0 bases"),
        ("a unit too long", dict(unit=b"A" * 4097, reads=r8, read_off=[0, 8]), "4097 bases"),
        ("a lower-case unit byte", dict(unit=b"ACgT", reads=r8, read_off=[0, 8]), "unit byte 2"),
        ("an N in the unit", dict(unit=b"NACG", reads=r8, read_off=[0, 8]), "unit byte 0"),
        ("match 0", dict(unit=u, reads=r8, read_off=[0, 8], match=0), "at least 1"),
        ("mismatch 0", dict(unit=u, reads=r8, read_off=[0, 8], mismatch=0), "at least 1"),
        ("gap -1", dict(unit=u, reads=r8, read_off=[0, 8], gap=-1), "at least 1"),
        ("scores beyond int32", dict(unit=u, reads=r8, read_off=[0, 8], match=1 << 28), "2\\^31"),
    ]


def check_refusals(eng, DeviceError):
    import ctypes as C
    import pytest
    u, r = b"ACGTTGCC", b"GGACGTTGCCACGTTGCCTT"
    wants = check(eng, u, [r, b"NN"])
    ptr0, ops0 = eng.ualign_ops()
    live = eng.stats()["hbm_bytes_live"]
    info0 = eng.ualign_info()
    for name, kw, msg in refusals():
        with pytest.raises(DeviceError, match=msg):
            eng.ualign_run(**kw)
        assert eng.stats()["hbm_bytes_live"] == live, name
        ptr, ops = eng.ualign_ops()
        assert np.array_equal(ptr, ptr0) and np.array_equal(ops, ops0), name
        i = eng.ualign_info()
        assert {k: v for k, v in i.items() if k != "phase_ms"} == {k: v for k, v in info0.items() if k != "phase_ms"}, name
    # null pointers
    lib, ctx = eng._lib, eng._ctx
    off = np.array([0, 4], np.int64)
    hits = np.zeros(1, eng.UALIGN_DTYPE)
    r8 = np.frombuffer(b"ACGT", np.uint8)
    u8 = np.frombuffer(b"ACGT", np.uint8)
    for args in ((None, 4, r8.ctypes.data, off.ctypes.data, 1, 10, 35, 33, hits.ctypes.data, None),
                 (u8.ctypes.data, 4, None, off.ctypes.data, 1, 10, 35, 33, hits.ctypes.data, None),
                 (u8.ctypes.data, 4, r8.ctypes.data, None, 1, 10, 35, 33, hits.ctypes.data, None),
                 (u8.ctypes.data, 4, r8.ctypes.data, off.ctypes.data, 1, 10, 35, 33, None, None)):
        assert lib.cf_ualign_run(ctx, *args) == -22
        assert eng.stats()["hbm_bytes_live"] == live
    assert lib.cf_ualign_info(ctx, None) == -22 and lib.cf_ualign_run(None, *args) == -22
    n = C.c_int64()
    assert lib.cf_ualign_ops(ctx, ptr0.ctypes.data, None, 0, C.byref(n)) == (-22 if ops0.size else 0) and n.value == ops0.size
    ptr, ops = eng.ualign_ops()
    assert np.array_equal(ptr, ptr0) and np.array_equal(ops, ops0)
    assert same(eng.ualign_run(u, np.frombuffer(r, np.uint8), [0, len(r)])[0][0], ops0[:ptr0[1]], wants[0])
    # no read at all, and empty reads only
    hits, ptr, ops = eng.ualign_run(u, np.zeros(0, np.uint8), [0])
    assert hits.size == 0 and ptr.tolist() == [0] and ops.size == 0
    hits, ptr, ops = eng.ualign_run(u, np.zeros(0, np.uint8), [0, 0, 0])
    assert hits.size == 2 and not hits["status"].any() and ptr.tolist() == [0, 0, 0]
    assert eng.stats()["hbm_bytes_live"] == live


def check_hygiene(eng, DeviceError, batch_bytes=(0, 0)):
    """two rounds of calls, refusals among them, leave the same live bytes and the same results; a round begins under its ualign_batch_bytes"""
    import pytest
    rng = np.random.default_rng(21)
    u = rand_seq(rng, 70)
    reads = [tandem_read(rng, u, 150, q & 1, 10) for q in range(5)] + [b""]
    rounds = []
    for first in batch_bytes:
        with eng.knobs(ualign_batch_bytes=first):
            wants = check(eng, u, reads)
            with pytest.raises(DeviceError):
                eng.ualign_run(b"ACGN", np.frombuffer(b"ACGT", np.uint8), [0, 4])
        with eng.knobs(ualign_batch_bytes=500):
            check(eng, u, reads, wants=wants)
        hits, ptr, ops = device(eng, u, reads)
        rounds.append((eng.stats()["hbm_bytes_live"], hits.tobytes(), ptr.tobytes(), ops.tobytes()))
    assert rounds[0] == rounds[1]


# ---------------------------------------------------------------- the report
FIRST_LINE = re.compile(r"^([^ ]+)\s+(\d+)\s+(\d+)bp\s+(\d+)-(\d+)\s+(.+)$")      # the reference's two expressions (scripts/ncrf_parser.py:74-75)
SECOND_LINE = re.compile(r"^([^+-]+)([+-])\s+(\d+)bp\s+score=(\d+)\s+(.+)$")


def header_line(scores):
    return f"# aligner=builtin match={scores[0]} mismatch={scores[1]} gap={scores[2]}\n"


def record_text(r_id, r_len, unit, w):
    return (f"{r_id} {r_len} {w['r_en'] - w['r_st']}bp {w['r_st']}-{w['r_en']} {w['r_al'].decode('latin-1')}\n"
            f"{unit.decode()}{'+-'[w['strand']]} {w['m_al_len']}bp score={w['score']} {w['m_al'].decode()}\n\n")


def report_text(unit, named_reads, scores=DEFAULT, min_length=500, aligner=align_np):
    out = [header_line(scores)]
    wants = []
    for name, seq in named_reads:
        w = aligner(unit, seq, scores)
        wants.append(w)
        if w is not None and w["r_en"] - w["r_st"] >= min_length:
            out.append(record_text(name, len(seq), unit, w))
    return "".join(out), wants


def parse_records(text):
    lines = [x.strip() for x in text.split("\n")]
    lines = [x for x in lines if x and x[0] != "#"]
    assert len(lines) % 2 == 0
    return [(FIRST_LINE.search(a).groups(), SECOND_LINE.search(b).groups()) for a, b in zip(lines[::2], lines[1::2])]


def reads_of_fixture(report_path, seed, flank=300):
    """(unit, [(name, read bytes)], {name: [(true start, true end) of each array stretch]}): the de-gapped r_al of every record of the
    fixture's report, in file orientation, records of one read id joined in r_st order, between random flanks."""
    with open(report_path) as f:
        recs = parse_records(f.read())
    rng = np.random.default_rng(seed)
    by_id, unit = {}, None
    for (r_id, r_len, r_al_len, r_st, r_en, r_al), (motif, strand, m_al_len, score, m_al) in recs:
        unit = unit or motif.encode()
        assert motif.encode() == unit
        by_id.setdefault(r_id, []).append((int(r_st), r_al.replace("-", "").encode(), strand, m_al))
    reads, truth = [], {}
    for r_id, parts in by_id.items():
        parts.sort(key=lambda p: p[0])
        seq, spans = rand_seq(rng, flank), []
        for _, b, strand, m_al in parts:
            spans.append((len(seq), len(seq) + len(b), strand, m_al))
            seq += b
        reads.append((r_id, seq + rand_seq(rng, flank)))
        truth[r_id] = spans
    return unit, reads, truth


def write_fasta(path, named):
    with open(path, "w") as f:
        for name, seq in named:
            f.write(f">{name}\n{seq.decode('latin-1')}\n")


def check_report(text, unit, named_reads, scores=DEFAULT, min_length=500):
    """checks 1 - 4 of the command line's report; returns the restatement's records"""
    want_text, wants = report_text(unit, named_reads, scores, min_length)
    assert text == want_text
    recs = parse_records(text)
    seqs = dict(named_reads)
    assert text.startswith(header_line(scores)) and text.count("#") == 1
    for (r_id, r_len, r_al_len, r_st, r_en, r_al), (motif, strand, m_al_len, score, m_al) in recs:
        read = seqs[r_id]
        r_st, r_en = int(r_st), int(r_en)
        assert int(r_len) == len(read) and int(r_al_len) == r_en - r_st >= min_length and len(r_al) == len(m_al)
        assert r_al.replace("-", "").encode("latin-1") == read[r_st:r_en]
        us = rc(unit) if strand == "-" else unit
        bases = m_al.replace("-", "").encode()
        assert motif.encode() == unit and int(m_al_len) == len(bases) and int(score) > 0
        ph = us.find(bases[:1]) if len(unit) < 4 else next(p for p in range(len(us)) if all(us[(p + k) % len(us)] == b for k, b in enumerate(bases[:40])))
        assert all(us[(ph + k) % len(us)] == b for k, b in enumerate(bases))
    return wants


# ---------------------------------------------------------------- the command line end to end
FIXTURE_SEED = {"tiny": 101, "hor2055": 102}
# Quality constants.  They are deterministic properties of the rule on the two fixtures' rebuilt reads (seeds above, flanks of 300
# random bases), computed on the CPU with the restatement alone (align_np) and asserted as the observed maxima; the device has to
# equal the restatement anyway.  END_SLACK: how far r_st / r_en lie from the true array ends 300 and len - 300 (a flank base
# continues the alignment only by chance, an error next to the end is cut off).  UNIT_SLACK: by how many units the split of the
# report's record (get_motif_alignments(1)) differs from the split of the fixture's own record of the same read, (over the reads
# the fixture has ONE record of, over all reads): a read the fixture has several records of is rebuilt from all of them, the
# aligner takes it in one stretch where the score allows, and the parser keeps only the fixture's longest record of it.
END_SLACK = {"tiny": 15, "hor2055": 22}
UNIT_SLACK = {"tiny": (1, 30), "hor2055": (0, 1)}


def quality(report_path, fixture_report, named_reads, flank=300):
    """(largest distance of an interval end from the true array end, (largest difference in units over the reads with one fixture
    record, over all reads)) over the records of the report"""
    from centroflye_amd.ncrf_parser import NCRF_Report
    with open(report_path, "rb") as f:
        recs = parse_records(f.read().decode("latin-1"))
    with open(fixture_report) as f:
        n_fixture = {}
        for a, _ in parse_records(f.read()):
            n_fixture[a[0]] = n_fixture.get(a[0], 0) + 1
    lens = {n: len(s) for n, s in named_reads}
    end = max(max(abs(int(a[3]) - flank), abs(int(a[4]) - (lens[a[0]] - flank))) for a, _ in recs)
    ours = NCRF_Report(report_path).get_motif_alignments(1)
    theirs = NCRF_Report(fixture_report).get_motif_alignments(1)
    diff = {r: abs(len(ours[r]) - len(theirs[r])) for r in ours if r in theirs}
    return end, (max(d for r, d in diff.items() if n_fixture[r] == 1), max(diff.values()))

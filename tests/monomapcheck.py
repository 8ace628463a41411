"""The rule of cf_monomap_run (include/cfhip.h) restated in plain Python — the reference's map_reads in spirit: a dict over
the slices of the edges, a slice at every read position, groupby — and what compares the device with it.  The restatement is pinned
by literal cases with every hit, path and flag written out (tests/test_emu_monomap.py) and by planted misreadings that each change a
literal.  The checks below are shared by the emulator suite and the GPU suite."""
import ctypes as C
from itertools import groupby

import numpy as np

GAP = b"?"


def restate(edges, uv, reads, k, gap=GAP, wrong=None):
    """per read ([(e, j, i) of every hit, ascending i], [the path's edges], valid).  wrong: one of WRONG_RULES, a planted misreading."""
    g = gap[0]
    crossing = wrong == "a window crosses a gap"
    index = {}
    for e, x in enumerate(edges):
        for j in range(len(x) - k + 1):
            w = x[j:j + k]
            if g in w and not crossing:
                continue
            index.setdefault(w, []).append((e, j))
    if wrong == "the first of a duplicate is kept":
        unique = {w: v[0] for w, v in index.items()}
    elif wrong == "unique per edge":
        unique = {}
        for w, v in index.items():
            once = [p for p in v if sum(q[0] == p[0] for q in v) == 1]
            if once:
                unique[w] = once[0]
    else:
        unique = {w: v[0] for w, v in index.items() if len(v) == 1}
    out, last_edge = [], None
    for x in reads:
        seen = []      # per window: a hit, or None
        for i in range(len(x) - k + 1):
            w = x[i:i + k]
            if g in w and not crossing:
                seen.append(None)
                continue
            at = unique.get(w)
            if at is None:
                seen.append(None)
                continue
            if wrong == "the position is relative to the piece":
                i -= x.rfind(gap, 0, i) + 1
            seen.append(at + (i,))
        hits = [h for h in seen if h is not None]
        if wrong == "a miss splits a run":
            path = [e for e, _ in groupby(None if h is None else h[0] for h in seen) if e is not None]
        elif wrong == "the path is a set":
            path = list(dict.fromkeys(h[0] for h in hits))
        else:
            path = [e for e, _ in groupby(h[0] for h in hits)]
        if wrong == "a run crosses the read border" and path and path[0] == last_edge:
            path = path[1:]
        if hits:
            last_edge = hits[-1][0]
        pairs = list(zip(path, path[1:]))
        if wrong == "validity on the first pair only":
            pairs = pairs[:1]
        out.append((hits, path, all(uv[a][1] == uv[b][0] for a, b in pairs)))
    return out


WRONG_RULES = ("the first of a duplicate is kept", "unique per edge", "a miss splits a run", "the path is a set", "a run crosses the read border",
               "validity on the first pair only", "the position is relative to the piece", "a window crosses a gap")

# (name, edges, (u, v) per edge, reads, k, per read (hits, path, valid))
LITERALS = [
    ("a k-mer twice in one edge is not indexed, at its first place neither", [b"ABABABC"], [(0, 1)], [b"ABABC"], 2,
     [([(0, 5, 3)], [0], True)]),
    ("a k-mer once in each of two edges is not indexed", [b"ABC", b"XBCY"], [(0, 1), (1, 2)], [b"ABCY"], 2,
     [([(0, 0, 0), (1, 2, 2)], [0, 1], True)]),
    ("a k-mer only in the reads", [b"ABC"], [(0, 1)], [b"XYZ", b"BCX"], 2,
     [([], [], True), ([(0, 1, 0)], [0], True)]),
    ("a k-mer only in the edges", [b"ABCD", b"EFG"], [(0, 1), (1, 2)], [b"EF"], 2,
     [([(1, 0, 0)], [1], True)]),
    ("hit, miss, hit on one edge: one run", [b"ABCDE"], [(0, 1)], [b"ABXDE"], 2,
     [([(0, 0, 0), (0, 3, 3)], [0], True)]),
    ("A-B-A stays three elements", [b"ABC", b"DEF"], [(0, 1), (1, 0)], [b"ABDEBC"], 2,
     [([(0, 0, 0), (1, 0, 2), (0, 1, 4)], [0, 1, 0], True)]),
    ("a self-loop edge", [b"XYZ", b"PQ"], [(0, 0), (0, 1)], [b"XYZPQ", b"PQXY"], 2,
     [([(0, 0, 0), (0, 1, 1), (1, 0, 3)], [0, 1], True), ([(1, 0, 0), (0, 0, 2)], [1, 0], False)]),
    ("an invalid join behind a valid one", [b"ABC", b"DEF", b"GHI"], [(0, 1), (1, 2), (5, 6)], [b"ABDEGH"], 2,
     [([(0, 0, 0), (1, 0, 2), (2, 0, 4)], [0, 1, 2], False)]),
    ("the last hit of one read and the first hit of the next on one edge", [b"ABCD", b"EF"], [(0, 1), (1, 2)], [b"EFAB", b"CDEF"], 2,
     [([(1, 0, 0), (0, 0, 2)], [1, 0], False), ([(0, 2, 0), (1, 0, 2)], [0, 1], True)]),
    ("a window beside a gap; the position counts the gap", [b"ABCD"], [(0, 1)], [b"AB?CD"], 2,
     [([(0, 0, 0), (0, 2, 3)], [0], True)]),
    ("positions behind gaps", [b"ABC", b"DE"], [(0, 1), (1, 2)], [b"?AB??DE"], 2,
     [([(0, 0, 1), (1, 0, 5)], [0, 1], True)]),
    ("an edge window with a gap equals no read window", [b"AB?CD"], [(0, 1)], [b"B?C", b"AB?CD"], 3,
     [([], [], True), ([], [], True)]),
    ("a read shorter than k, and one of exactly k", [b"ABCD"], [(0, 1)], [b"AB", b"ABC"], 3,
     [([], [], True), ([(0, 0, 0)], [0], True)]),
    ("empty reads", [b"ABC"], [(0, 1)], [b"", b"BC", b""], 2,
     [([], [], True), ([(0, 1, 0)], [0], True), ([], [], True)]),
    ("E = 0", [], [], [b"ABC", b""], 2,
     [([], [], True), ([], [], True)]),
    ("R = 0", [b"ABC"], [(0, 1)], [], 2, []),
    ("k = 1", [b"ABCA", b"D"], [(0, 1), (1, 2)], [b"BADC?D"], 1,
     [([(0, 1, 0), (1, 0, 2), (0, 2, 3), (1, 0, 5)], [0, 1, 0, 1], False)]),
    ("another gap byte", [b"AB?C"], [(0, 1)], [b"B?C-AB"], 2,
     [([(0, 1, 0), (0, 2, 1), (0, 0, 4)], [0], True)]),
    ("an empty edge and an edge shorter than k", [b"", b"A", b"ABC"], [(0, 1), (1, 2), (2, 3)], [b"ABC"], 2,
     [([(2, 0, 0), (2, 1, 1)], [2], True)]),
]
LITERAL_GAPS = {"another gap byte": b"-"}


def check_literal(name, edges, uv, reads, k, want, wrong=None):
    return restate(edges, uv, reads, k, LITERAL_GAPS.get(name, GAP), wrong) == want


def killers():
    """misreading -> the literal cases it changes"""
    return {w: [c[0] for c in LITERALS if not check_literal(*c, wrong=w)] for w in WRONG_RULES}


# ---------------------------------------------------------------- device == restatement (shared by the emulator and the GPU suite)
def device_result(eng, edges, uv, reads, k, gap=GAP):
    """the device's answer in the restatement's form, with every per-read field checked against the two CSRs on the way"""
    info, (ptr, path), (hptr, hits) = eng.monomap(edges, uv, reads, k, gap, hits=True)
    n = len(reads)
    assert len(info) == n and len(ptr) == n + 1 == len(hptr) and ptr[0] == 0 == hptr[0] and ptr[-1] == len(path) and hptr[-1] == len(hits)
    bare, (ptr2, path2) = eng.monomap(edges, uv, reads, k, gap)
    assert np.array_equal(bare, info) and np.array_equal(ptr, ptr2) and np.array_equal(path, path2)
    assert eng.monomap_info()["with_hits"] == 0
    out = []
    hit_rows, path_list = hits.tolist(), path.tolist()
    for r, rec in enumerate(info.tolist()):
        n_hits, e0, j0, i0, e1, j1, i1, valid, n_path = rec
        hl = [tuple(h) for h in hit_rows[hptr[r]:hptr[r + 1]]]
        pl = path_list[ptr[r]:ptr[r + 1]]
        assert n_hits == len(hl) and n_path == len(pl) and valid in (0, 1)
        assert (e0, j0, i0) == (hl[0] if hl else (-1, -1, -1)) and (e1, j1, i1) == (hl[-1] if hl else (-1, -1, -1))
        out.append((hl, pl, bool(valid)))
    return out


def check(eng, edges, uv, reads, k, gap=GAP, want=None):
    """every field of the device's answer equals the restatement's, with and without the hits; _info's figures too"""
    want = restate(edges, uv, reads, k, gap) if want is None else want
    got = device_result(eng, edges, uv, reads, k, gap)
    small = sum(map(len, edges)) + sum(map(len, reads)) < 200
    for r, (a, b) in enumerate(zip(got, want)):
        assert a == b, (r, (edges, uv, reads) if small else "...", k, a if small else (a[0][:5], a[1][:5], a[2]), b if small else (b[0][:5], b[1][:5], b[2]))
    assert len(got) == len(want)
    info = eng.monomap_info()
    g = gap[0]
    windows = [x[j:j + k] for x in edges for j in range(len(x) - k + 1) if g not in x[j:j + k]]
    counts = {}
    for w in windows:
        counts[w] = counts.get(w, 0) + 1
    assert info["n_edges"] == len(edges) and info["n_reads"] == len(reads) and info["k"] == k
    assert info["n_edge_letters"] == sum(map(len, edges)) and info["n_read_letters"] == sum(map(len, reads))
    n = info["n_edge_letters"] + info["n_read_letters"]
    if 0 < n and k <= n:
        assert info["n_edge_windows"] == len(windows) and info["n_indexed"] == sum(c == 1 for c in counts.values())
        rounds = (k.bit_length() - 1) + (1 if k & (k - 1) else 0)
        assert info["n_rounds"] == rounds and info["n_sorts"] <= max(rounds, 1)
    assert info["n_hits"] == sum(len(h) for h, _, _ in want) and info["n_path"] == sum(len(p) for _, p, _ in want)
    return want


def check_literals(eng):
    for name, edges, uv, reads, k, want in LITERALS:
        check(eng, edges, uv, reads, k, LITERAL_GAPS.get(name, GAP), want)


def cut(text, n_pieces, rng):
    """text cut at n_pieces - 1 random places (pieces may be empty)"""
    at = sorted(int(x) for x in rng.integers(0, len(text) + 1, n_pieces - 1))
    return [text[a:b] for a, b in zip([0] + at, at + [len(text)])]


def graph_like(rng, n_edge_letters, n_read_letters, n_edges=4, n_reads=5, letters=b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", gap_rate=0.01, sub_rate=0.02, piece=40):
    """edges of random letters, and reads that are pieces of the edges' text back to back with a few wrong letters and gaps: exactly
    n_edge_letters and n_read_letters letters in all; the nodes are drawn from four, so that joins hold and break"""
    text = rng.choice(np.frombuffer(letters, np.uint8), n_edge_letters).tobytes()
    edges = cut(text, n_edges, rng)
    uv = [(int(a), int(b)) for a, b in rng.integers(0, 4, (len(edges), 2))]
    out = bytearray()
    while len(out) < n_read_letters and n_edge_letters:
        a = int(rng.integers(0, n_edge_letters))
        out += text[a:a + int(rng.integers(1, piece + 1))]
    out = np.frombuffer(bytes(out[:n_read_letters]) + b"A" * (n_read_letters - len(out)), np.uint8).copy()
    m = rng.random(len(out)) < sub_rate
    out[m] = rng.choice(np.frombuffer(letters, np.uint8), int(m.sum()))
    out[rng.random(len(out)) < gap_rate] = GAP[0]
    return edges, uv, cut(out.tobytes(), n_reads, rng)


def check_small_seeded(eng, n_cases=40, seed=7):
    rng = np.random.default_rng(seed)
    hits = 0
    for c in range(n_cases):
        edges, uv, reads = graph_like(rng, int(rng.integers(0, 30)), int(rng.integers(0, 40)), int(rng.integers(1, 5)), int(rng.integers(1, 5)),
                                      b"AB" if c % 3 == 0 else b"ABCDEF", 0.08, 0.05, 9)
        hits += sum(len(h) for h, _, _ in check(eng, edges, uv, reads, int(rng.integers(1, 5))))
    assert hits > n_cases


ALL_K = (1, 2, 3, 5, 8, 9, 255, 256, 257)


def check_all_k(eng, seed=0, n_edge_letters=1500, n_read_letters=1800):
    """no round, one round, the overlapping combine, powers of two and their neighbours; reads that follow the edges for hundreds of letters"""
    rng = np.random.default_rng(seed)
    edges, uv, reads = graph_like(rng, n_edge_letters, n_read_letters, 3, 4, b"ABCD", 0.001, 0.001, 700)
    edges, uv, reads = edges + [b"WXYZ"], uv + [(1, 1)], reads + [b"AWXYZWXYZA"]      # (letters that occur once, for the small k)
    for k in ALL_K:
        want = check(eng, edges, uv, reads, k)
        assert sum(len(h) for h, _, _ in want) > 0, k
    return edges, uv, reads


def check_borders(eng, sizes, k=3):
    """the edge letters (and so the edge/read border of the concatenation), the read letters and the number of hits on the borders of
    the sort's tile, the scan's tile and the streaming passes' block"""
    rng = np.random.default_rng(11)
    for n in sizes:
        edges, uv, reads = graph_like(rng, n, n + 77, 3, 4)
        check(eng, edges, uv, reads, k)                       # the border of the concatenation at n
        edges, uv, reads = graph_like(rng, 3 * n // 2, n, 2, 3)
        check(eng, edges, uv, reads, k - 1)                   # n read letters
        check(eng, [text for text in edges], uv, [b"".join(reads)], k)
        # exactly n hits, in one run and in n runs; the last read window is a hit
        want = check(eng, [b"A", b"B", b"CC"], [(0, 1), (1, 0), (1, 1)], [b"C" + b"A" * n, b"", (b"AB" * n)[:n]], 1)
        assert [len(h) for h, _, _ in want] == [n, 0, n] and [len(p) for _, p, _ in want] == [1, 0, n] and want[2][2]
        want = check(eng, [b"XAAY"], [(0, 1)], [b"XAAY" * (n // 3), b"XAA"[:n % 3 + 1] if n % 3 else b""], 2)
        assert sum(len(h) for h, _, _ in want) == n


def check_lengths_against_k(eng):
    for edges, reads, k in (([b"ABCAB"], [b"ABCAB"], 5), ([b"ABCAB"], [b"ABCAB"], 6), ([b"ABC"], [b"AB", b"ABC"], 9), ([b"A"], [b"A"], 1), ([b"A"], [b"A"], 2),
                            ([b""], [b""], 1), ([], [], 1), ([b"", b""], [b"", b"", b""], 3), ([b"????"], [b"??"], 2), ([b"?A?"], [b"A", b"?"], 1),
                            ([b"ABCD"], [], 2), ([], [b"ABCD"], 2), ([b"AB"], [b"ABCDEFG"], 3), ([b"ABCDEFG"], [b"AB"], 3)):
        check(eng, edges, [(s, s + 1) for s in range(len(edges))], reads, k)


# ---------------------------------------------------------------- large shapes: compared through numpy, not the dict (k <= 8)
def pack(strings, k, gap):
    """the valid windows of k <= 8 letters as integers: (keys uint64, string index, index in the string), in ascending (s, i)"""
    keys, where = [np.zeros(0, np.uint64)], [np.zeros((0, 2), np.int64)]
    for s, x in enumerate(strings):
        a = np.frombuffer(x, np.uint8).astype(np.uint64)
        n = len(a) - k + 1
        if n < 1:
            continue
        key, ok = np.zeros(n, np.uint64), np.ones(n, bool)
        for j in range(k):
            key = (key << np.uint64(8)) | a[j:j + n]
            ok &= a[j:j + n] != gap[0]
        idx = np.nonzero(ok)[0]
        keys.append(key[idx])
        where.append(np.stack([np.full(len(idx), s, np.int64), idx.astype(np.int64)], 1))
    return np.concatenate(keys), np.concatenate(where)


def restate_np(edges, uv, reads, k, gap=GAP):
    """the same rule with numpy: (hits (read, e, j, i) in output order, per read n_hits, n_path, valid, and the paths' edges)"""
    assert k <= 8
    ek, ew = pack(edges, k, gap)
    rk, rw = pack(reads, k, gap)
    vals, first, counts = np.unique(ek, return_index=True, return_counts=True)
    vals, first = vals[counts == 1], first[counts == 1]
    at = np.searchsorted(vals, rk)
    ok = at < len(vals)
    ok[ok] = vals[at[ok]] == rk[ok]
    place = ew[first[at[ok]]]
    hits = np.stack([rw[ok, 0], place[:, 0], place[:, 1], rw[ok, 1]], 1) if ok.any() else np.zeros((0, 4), np.int64)
    head = np.ones(len(hits), bool)
    head[1:] = (hits[1:, 0] != hits[:-1, 0]) | (hits[1:, 1] != hits[:-1, 1])
    uv = np.asarray(uv, np.int64).reshape(-1, 2)
    broken = np.zeros(len(hits), bool)
    broken[1:] = head[1:] & (hits[1:, 0] == hits[:-1, 0]) & (uv[hits[:-1, 1], 1] != uv[hits[1:, 1], 0])
    n = len(reads)
    n_hits = np.bincount(hits[:, 0], minlength=n)
    n_path = np.bincount(hits[head, 0], minlength=n)
    valid = np.bincount(hits[broken, 0], minlength=n) == 0
    return hits, n_hits, n_path, valid, hits[head, 1]


def check_np(eng, edges, uv, reads, k, gap=GAP):
    hits, n_hits, n_path, valid, path = restate_np(edges, uv, reads, k, gap)
    info, (ptr, got_path), (hptr, got) = eng.monomap(edges, uv, reads, k, gap, hits=True)
    assert np.array_equal(info["n_hits"], n_hits) and np.array_equal(info["n_path"], n_path) and np.array_equal(info["valid"] != 0, valid)
    assert np.array_equal(np.diff(hptr), n_hits) and np.array_equal(np.diff(ptr), n_path) and hptr[0] == 0 == ptr[0]
    assert np.array_equal(got["e"], hits[:, 1]) and np.array_equal(got["j"], hits[:, 2]) and np.array_equal(got["i"], hits[:, 3])
    assert np.array_equal(got_path, path)
    some = n_hits > 0
    for name, col, at in (("e0", 1, hptr[:-1]), ("j0", 2, hptr[:-1]), ("i0", 3, hptr[:-1]), ("e1", 1, hptr[1:] - 1), ("j1", 2, hptr[1:] - 1), ("i1", 3, hptr[1:] - 1)):
        assert np.array_equal(info[name][some], hits[at[some], col]) and np.all(info[name][~some] == -1)
    stats = eng.monomap_info()
    assert stats["n_hits"] == len(hits) and stats["n_path"] == len(path)
    return stats


def check_many_reads(eng, n_reads):
    """more reads than a launch has threads: one or two letters each, k = 1"""
    rng = np.random.default_rng(13)
    pool = [b"A", b"B", b"AB", b"BA", b"?", b"C?", b"AC", b"D"]
    reads = [pool[int(x)] for x in rng.integers(0, len(pool), n_reads)]
    stats = check_np(eng, [b"AB", b"C", b"DD"], [(0, 1), (1, 2), (2, 0)], reads, 1)
    assert stats["n_reads"] == n_reads and stats["n_indexed"] == 3 and stats["n_hits"] > n_reads // 2


def check_long_run(eng, n=200000):
    """a read of n equal letters against an edge that holds the letter once: n hits, one run"""
    info, (ptr, path), (hptr, hits) = eng.monomap([b"XAY", b"Z"], [(0, 1), (1, 2)], [b"Z", b"A" * n, b"ZA"], 1, hits=True)
    assert info.tolist() == [(1, 1, 0, 0, 1, 0, 0, 1, 1), (n, 0, 1, 0, 0, 1, n - 1, 1, 1), (2, 1, 0, 0, 0, 1, 1, 0, 2)]
    assert ptr.tolist() == [0, 1, 2, 4] and path.tolist() == [1, 0, 1, 0] and hptr.tolist() == [0, 1, n + 1, n + 3]
    assert np.all(hits["e"][1:n + 1] == 0) and np.all(hits["j"][1:n + 1] == 1) and np.array_equal(hits["i"][1:n + 1], np.arange(n, dtype=np.int32))


def check_refusals(eng, DeviceError):
    import pytest
    edges, uv, reads = [b"ABCDE", b"EFG"], [(0, 1), (1, 2)], [b"ABC?CDE", b"FG"]
    base = check(eng, edges, uv, reads, 2)
    eng.monomap(edges, uv, reads, 2, hits=True)
    live = eng.stats()["hbm_bytes_live"]
    last = eng.monomap_info()
    e_flat, r_flat = np.frombuffer(b"".join(edges), np.uint8), np.frombuffer(b"".join(reads), np.uint8)
    e_off, r_off = np.array([0, 5, 8], np.int64), np.array([0, 7, 9], np.int64)
    u, v = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731

    def refused(match, eb=e_flat, eo=e_off, uu=u, vv=v, ne=2, rb=r_flat, ro=r_off, nr=2, k=2, gap=63):
        with pytest.raises(DeviceError, match=match) as e:
            eng._check(eng._lib.cf_monomap_run(eng._ctx, p(eb), p(eo), p(uu), p(vv), ne, p(rb), p(ro), nr, k, gap, 1, None, None), "cf_monomap_run")
        assert "(-22)" in str(e.value)
        assert eng.stats()["hbm_bytes_live"] == live
        now = eng.monomap_info()
        assert {k_: v_ for k_, v_ in now.items() if k_ != "phase_ms"} == {k_: v_ for k_, v_ in last.items() if k_ != "phase_ms"}

    refused("k is below 1", k=0)
    refused("k is below 1", k=-3)
    refused("null edge bytes", eb=None)
    refused("null read bytes", rb=None)
    refused("null edge offsets", eo=None)
    refused("null read offsets", ro=None)
    refused("null edge nodes", uu=None)
    refused("null edge nodes", vv=None)
    refused("edge offsets do not ascend", eo=np.array([0, 5, 3], np.int64))
    refused("read offsets do not ascend", ro=np.array([0, 7, 6], np.int64))
    refused("negative edge offset", eo=np.array([-1, 5, 8], np.int64))
    refused("negative read offset", ro=np.array([-2, 7, 9], np.int64))
    refused("gap byte is outside", gap=256)
    refused("gap byte is outside", gap=-1)
    refused("number of edges is outside", ne=-1)
    refused("number of edges is outside", ne=1 << 31)
    refused("number of reads is outside", nr=-1)
    refused("number of reads is outside", nr=1 << 31)
    # N >= 2^31 is refused from the offsets alone, before a byte is read: each set alone, and the two together
    refused("2\\^31 or more", ro=np.array([0, 7, 1 << 31], np.int64))
    refused("2\\^31 or more", eo=np.array([0, 5, 1 << 31], np.int64))
    refused("2\\^31 or more", eo=np.array([0, 5, 1 << 30], np.int64), ro=np.array([0, 7, 1 << 30], np.int64))
    # the results of the run before the refusals are still there
    n_path, n_hits = C.c_int64(), C.c_int64()
    eng._check(eng._lib.cf_monomap_get(eng._ctx, None, None, 0, C.byref(n_path), None, None, 0, C.byref(n_hits)), "cf_monomap_get")
    assert n_path.value == sum(len(q) for _, q, _ in base) and n_hits.value == sum(len(h) for h, _, _ in base) > 0
    # positive counts with null pointers are refused; with no string the pointers may be null
    eng._check(eng._lib.cf_monomap_run(eng._ctx, None, None, None, None, 0, None, None, 0, 2, 63, 0, None, None), "cf_monomap_run")
    assert eng.stats()["hbm_bytes_live"] == live and eng.monomap_info()["n_hits"] == 0
    eng.monomap(edges, uv, reads, 2)
    with pytest.raises(DeviceError, match="room for 0 path elements"):
        eng._check(eng._lib.cf_monomap_get(eng._ctx, None, (C.c_int32 * 1)(), 0, None, None, None, 0, None), "cf_monomap_get")
    with pytest.raises(DeviceError, match="kept no hits"):
        eng._check(eng._lib.cf_monomap_get(eng._ctx, None, None, 0, None, (C.c_int64 * 3)(), None, 0, None), "cf_monomap_get")


def check_hygiene(eng):
    rng = np.random.default_rng(41)
    edges, uv, reads = graph_like(rng, 300, 400)
    a = eng.monomap(edges, uv, reads, 3, hits=True)
    live = eng.stats()["hbm_bytes_live"]
    t0, s0 = eng.times(), dict(eng.stats())
    b = eng.monomap(edges, uv, reads, 3, hits=True)
    assert eng.stats()["hbm_bytes_live"] == live
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))
    assert len(a[2][1]) > 50
    check(eng, edges, uv, reads, 3)
    assert eng.times() == t0 and eng.stats() == s0      # nothing is added to cf_times or cf_stats


def check_get_before_run(eng, DeviceError):
    import pytest
    n = C.c_int64()
    with pytest.raises(DeviceError, match="no cf_monomap_run before"):
        eng._check(eng._lib.cf_monomap_get(eng._ctx, None, None, 0, C.byref(n), None, None, 0, None), "cf_monomap_get")
    info, (ptr, path) = eng.monomap([b"ABC"], [(0, 1)], [b"BCAB"], 2)
    assert info.tolist() == [(2, 0, 1, 0, 0, 0, 2, 1, 1)] and ptr.tolist() == [0, 1] and path.tolist() == [0]

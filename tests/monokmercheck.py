"""The rule of cf_monokmers_run (include/cfhip.h) restated in plain Python — the reference's loop in spirit: a dict over
slices — and what compares the device with it.  The reference has only its Python loop behind the rule (scripts/debruijn_graph.py
get_frequent_kmers / read_kmer_locations), so the restatement is pinned by literal cases with every k-mer, count, first position
and occurrence list written out (tests/test_emu_monokmers.py), and by planted misreadings that each change a literal.  The checks
below are shared by the emulator suite and the GPU suite."""
import numpy as np

GAP = b"?"


def restate(strings, k, min_mult, gap=GAP, wrong=None):
    """[(k-mer bytes, count, (s, i) of the first window, [(s, i) of every window, ascending])] in the order of first occurrence.
    wrong: one of WRONG_RULES, a planted misreading."""
    g = gap[0]
    if wrong == "across the border":
        strings = [b"".join(strings)]
    occ = {}
    for s, x in enumerate(strings):
        for i in range(len(x) - k + 1):
            w = x[i:i + k]
            body = w[:-1] if wrong == "gap at the last byte" else w
            if g in body:
                continue
            if wrong == "stale table" and k & (k - 1):
                # the last combine read as (R_a[p], R_{k-a}[p + a]) with the table of the round before, which holds ranks of length
                # a / 2 where it should hold k - a letters: the tail is compared on a / 2 letters, fewer or more than it has
                a = 1 << (k.bit_length() - 1)
                w = w[:a] + b"|" + x[i + a:i + a + a // 2]
            occ.setdefault(w, []).append((s, i))
    out = [(w, len(v), v[0], list(v)) for w, v in occ.items() if (len(v) > min_mult if wrong == "greater than" else len(v) >= min_mult)]
    if wrong == "by count":
        out.sort(key=lambda r: -r[1])
    if wrong == "by bytes":
        out.sort(key=lambda r: r[0])
    if wrong == "unsorted occurrences":
        out = [(w, c, f, v[::-1]) for w, c, f, v in out]
    if wrong == "stale table" and k & (k - 1):
        out = [(strings[f[0]][f[1]:f[1] + k], c, f, v) for w, c, f, v in out]
    return out


WRONG_RULES = ("across the border", "gap at the last byte", "by count", "by bytes", "greater than", "unsorted occurrences", "stale table")

# (name, strings, k, min_mult, the whole result)
LITERALS = [
    ("k = 1: every letter, the gap left out", [b"AB?A"], 1, 1,
     [(b"A", 2, (0, 0), [(0, 0), (0, 3)]), (b"B", 1, (0, 1), [(0, 1)])]),
    ("the order of first occurrence, neither by count nor by bytes", [b"CABABAB"], 2, 1,
     [(b"CA", 1, (0, 0), [(0, 0)]), (b"AB", 3, (0, 1), [(0, 1), (0, 3), (0, 5)]), (b"BA", 2, (0, 2), [(0, 2), (0, 4)])]),
    ("min_mult is met by exactly min_mult windows", [b"CABABAB"], 2, 2,
     [(b"AB", 3, (0, 1), [(0, 1), (0, 3), (0, 5)]), (b"BA", 2, (0, 2), [(0, 2), (0, 4)])]),
    ("min_mult - 1 windows are too few", [b"CABABAB"], 2, 3, [(b"AB", 3, (0, 1), [(0, 1), (0, 3), (0, 5)])]),
    ("two strings whose concatenation holds a k-mer that neither holds alone", [b"AB", b"CA", b"BC"], 2, 1,
     [(b"AB", 1, (0, 0), [(0, 0)]), (b"CA", 1, (1, 0), [(1, 0)]), (b"BC", 1, (2, 0), [(2, 0)])]),
    ("a gap at the first and at the last byte of a window, and directly beside it", [b"?ABC?ABC", b"ABC?"], 3, 1,
     [(b"ABC", 3, (0, 1), [(0, 1), (0, 5), (1, 0)])]),
    ("the overlapping combine: k = 3 on strings that agree on the first two letters", [b"ABCD", b"ABDD", b"ABCD"], 3, 1,
     [(b"ABC", 2, (0, 0), [(0, 0), (2, 0)]), (b"BCD", 2, (0, 1), [(0, 1), (2, 1)]), (b"ABD", 1, (1, 0), [(1, 0)]), (b"BDD", 1, (1, 1), [(1, 1)])]),
    ("k = 3: windows that differ only in their last letter", [b"AAB", b"AAC", b"AAB"], 3, 1,
     [(b"AAB", 2, (0, 0), [(0, 0), (2, 0)]), (b"AAC", 1, (1, 0), [(1, 0)])]),
    ("k = 5: equal windows with different letters behind them, and one that differs in its last letter", [b"ABCDEX", b"ABCDF", b"?ABCDEY"], 5, 1,
     [(b"ABCDE", 2, (0, 0), [(0, 0), (2, 1)]), (b"BCDEX", 1, (0, 1), [(0, 1)]), (b"ABCDF", 1, (1, 0), [(1, 0)]), (b"BCDEY", 1, (2, 2), [(2, 2)])]),
    ("k = 7: windows that differ only in their last letter", [b"ABCDEFG", b"ABCDEFH"], 7, 1,
     [(b"ABCDEFG", 1, (0, 0), [(0, 0)]), (b"ABCDEFH", 1, (1, 0), [(1, 0)])]),
    ("k = 6: tails that agree on two letters and differ behind them", [b"ABCDEFG", b"ABCDEFH", b"ABCDEF"], 6, 1,
     [(b"ABCDEF", 3, (0, 0), [(0, 0), (1, 0), (2, 0)]), (b"BCDEFG", 1, (0, 1), [(0, 1)]), (b"BCDEFH", 1, (1, 1), [(1, 1)])]),
    ("k = len, k = len + 1, an empty string and a string of one byte", [b"ABC", b"AB", b"", b"A", b"ABC"], 3, 1,
     [(b"ABC", 2, (0, 0), [(0, 0), (4, 0)])]),
    ("k larger than every string", [b"ABC", b"AB"], 4, 1, []),
    ("all gaps", [b"???", b"?"], 1, 1, []),
    ("no string at all", [], 2, 1, []),
    ("one string of equal letters: one class, every rank equal", [b"AAAAA"], 2, 1, [(b"AA", 4, (0, 0), [(0, 0), (0, 1), (0, 2), (0, 3)])]),
    ("another gap byte", [b"AB-AB?"], 2, 1, [(b"AB", 2, (0, 0), [(0, 0), (0, 3)]), (b"B?", 1, (0, 4), [(0, 4)])]),
]
LITERAL_GAPS = {"another gap byte": b"-"}


def check_literal(name, strings, k, min_mult, want, wrong=None):
    return restate(strings, k, min_mult, LITERAL_GAPS.get(name, GAP), wrong) == want


def killers():
    """misreading -> the literal cases it changes"""
    return {w: [c[0] for c in LITERALS if not check_literal(*c, wrong=w)] for w in WRONG_RULES}


# ---------------------------------------------------------------- device == restatement (shared by the emulator and the GPU suite)
def device_result(eng, strings, k, min_mult, gap=GAP, positions=True):
    """the device's answer in the restatement's form (the k-mer's letters cut at pos from the concatenation)"""
    flat = b"".join(strings)
    if positions:
        first, ptr, occ = eng.monokmers(strings, k, min_mult, True, gap)
        assert len(ptr) == len(first) + 1 and ptr[0] == 0 and ptr[-1] == len(occ)
        pairs = list(zip(occ["s"].tolist(), occ["i"].tolist()))
        lists = [pairs[ptr[j]:ptr[j + 1]] for j in range(len(first))]
    else:
        first = eng.monokmers(strings, k, min_mult, False, gap)
        lists = [None] * len(first)
    out = []
    for row, lst in zip(first.tolist(), lists):
        s, i, count, pos = row
        out.append((flat[pos:pos + k], count, (s, i), lst))
    return out


def check(eng, strings, k, min_mult, gap=GAP, want=None):
    """every field of the device's answer equals the restatement's, with and without the occurrence lists; _info's counts too"""
    want = restate(strings, k, min_mult, gap) if want is None else want
    got = device_result(eng, strings, k, min_mult, gap, True)
    assert got == want, (strings if sum(map(len, strings)) < 200 else "...", k, min_mult, got[:5], want[:5])
    info = eng.monokmers_info()
    everything = restate(strings, k, 1, gap)
    assert info["n_windows"] == sum(c for _, c, _, _ in everything) and info["n_distinct"] == len(everything)
    assert info["n_kmers"] == len(want) and info["n_occ"] == sum(c for _, c, _, _ in want) and info["with_positions"] == 1
    assert info["n_strings"] == len(strings) and info["n_letters"] == sum(map(len, strings)) and info["k"] == k
    n = sum(map(len, strings))
    if 0 < n and k <= n:
        rounds = (k.bit_length() - 1) + (1 if k & (k - 1) else 0)
        assert info["n_rounds"] == rounds
        assert info["n_sorts"] <= max(rounds, 1) + 1      # (the rounds stop at the first length that no window has)
    bare = device_result(eng, strings, k, min_mult, gap, False)
    assert [r[:3] for r in bare] == [r[:3] for r in want]
    assert eng.monokmers_info()["with_positions"] == 0 and eng.monokmers_info()["n_occ"] == 0
    return want


def check_literals(eng):
    for name, strings, k, min_mult, want in LITERALS:
        check(eng, strings, k, min_mult, LITERAL_GAPS.get(name, GAP), want)


def random_strings(rng, n_strings, max_len, letters=b"ABC", gap_rate=0.1):
    out = []
    for _ in range(n_strings):
        n = int(rng.integers(0, max_len + 1))
        x = rng.choice(np.frombuffer(letters, np.uint8), n)
        x[rng.random(n) < gap_rate] = GAP[0]
        out.append(x.tobytes())
    return out


def hor_strings(rng, n_strings, n_letters, period=12, sub=0.02, gaps=0.02):
    """strings that read one period cyclically from a random phase, with substitutions and gaps: many repeats of every k-mer"""
    hor = np.frombuffer(bytes(range(65, 65 + period)), np.uint8)
    out = []
    for _ in range(n_strings):
        n = int(rng.integers(n_letters // 2, n_letters + 1))
        x = hor[(int(rng.integers(0, period)) + np.arange(n)) % period].copy()
        m = rng.random(n) < sub
        x[m] = rng.integers(65, 65 + period, int(m.sum()))
        x[rng.random(n) < gaps] = GAP[0]
        out.append(x.tobytes())
    return out


ALL_K = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257)


def check_all_k(eng, seed=0, n_strings=5, n_letters=600):
    """no round, one round, the overlapping combine, powers of two and their neighbours, on periodic strings with errors"""
    rng = np.random.default_rng(seed)
    strings = hor_strings(rng, n_strings, n_letters, gaps=0.002) + [b"", b"A"]
    assert max(map(len, strings)) > 257
    seen = 0
    for k in ALL_K:
        for mm in (1, 2):
            seen += len(check(eng, strings, k, mm))
    assert seen > 0
    return strings


def check_small_seeded(eng, n_cases=40, seed=7):
    rng = np.random.default_rng(seed)
    for c in range(n_cases):
        strings = random_strings(rng, int(rng.integers(0, 6)), 12, b"AB" if c & 1 else b"ABC")
        check(eng, strings, int(rng.integers(1, 8)), int(rng.integers(1, 4)))


def check_lengths_against_k(eng):
    for strings, k in (([b"ABCAB"], 5), ([b"ABCAB"], 6), ([b"ABCAB", b"ABC"], 9), ([b"A"], 1), ([b"A"], 2), ([b""], 1), ([], 1), ([b"", b"", b""], 3),
                       ([b"????"], 2), ([b"?A?", b"A"], 1)):
        check(eng, strings, k, 1)


def check_borders(eng, sizes, k=3):
    """N on the borders of the sort's tile and of the streaming passes' block, in one string and in two"""
    rng = np.random.default_rng(11)
    for n in sizes:
        x = random_strings(rng, 1, n, b"ABCD", 0.03)[0]
        x = x + b"A" * (n - len(x))
        check(eng, [x], k, 2)
        check(eng, [x[:n // 3], x[n // 3:]], k + 1, 1)


def check_many_strings(eng, n_strings):
    """more strings than a launch has threads: single letters, pairs and empty strings"""
    rng = np.random.default_rng(13)
    pool = [b"A", b"B", b"AB", b"", b"BA", b"?", b"ABA"]
    strings = [pool[int(x)] for x in rng.integers(0, len(pool), n_strings)]
    check(eng, strings, 2, 1)
    check(eng, strings, 1, n_strings // 8)


def check_refusals(eng, DeviceError):
    import pytest
    strings = [b"ABCAB?ABC", b"CAB"]
    base = check(eng, strings, 3, 1)
    eng.monokmers(strings, 3, 1, True)
    live = eng.stats()["hbm_bytes_live"]
    last = eng.monokmers_info()
    flat = b"".join(strings)

    def refused(match, *args):
        with pytest.raises(DeviceError, match=match) as e:
            eng.monokmers(*args)
        assert "(-22)" in str(e.value)
        assert eng.stats()["hbm_bytes_live"] == live
        now = eng.monokmers_info()
        assert {k: v for k, v in now.items() if k != "phase_ms"} == {k: v for k, v in last.items() if k != "phase_ms"}

    refused("k is below 1", strings, 0, 1)
    refused("k is below 1", strings, -3, 1)
    refused("min_mult is below 1", strings, 3, 0)
    refused("do not ascend", (flat, np.array([0, 9, 5], np.int64)), 3, 1)
    refused("negative", (flat, np.array([-1, 9, 12], np.int64)), 3, 1)
    # N >= 2^31 is refused from the offsets alone, before a byte is read (the bytes here are never touched)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1 << 31,), strides=(0,))
    with pytest.raises(DeviceError, match="2\\^31 or more") as e:
        eng._check(eng._lib.cf_monokmers_run(eng._ctx, big.ctypes.data, np.array([0, 1 << 31], np.int64).ctypes.data, 1, 3, 1, 63, 0, None, None), "cf_monokmers_run")
    assert "(-22)" in str(e.value) and eng.stats()["hbm_bytes_live"] == live
    # the results of the run before the refusals are still there
    first, ptr, occ = eng.monokmers(strings, 3, 1, True)
    refused("k is below 1", strings, 0, 1)
    import ctypes as C
    n = C.c_int64()
    eng._check(eng._lib.cf_monokmers_get(eng._ctx, None, 0, C.byref(n), None, None, 0, None), "cf_monokmers_get")
    assert n.value == len(first) == len(base)


def check_hygiene(eng):
    rng = np.random.default_rng(41)
    strings = hor_strings(rng, 6, 80)
    a = eng.monokmers(strings, 5, 2, True)
    live = eng.stats()["hbm_bytes_live"]
    t0, s0 = eng.times(), dict(eng.stats())
    b = eng.monokmers(strings, 5, 2, True)
    assert eng.stats()["hbm_bytes_live"] == live
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    check(eng, strings, 5, 2)
    assert eng.times() == t0 and eng.stats() == s0      # nothing is added to cf_times or cf_stats


# ---------------------------------------------------------------- large shapes (GPU suite): compared through numpy, not the dict
def restate_np(strings, k, min_mult, gap=GAP):
    """the same rule with numpy (k <= 8, letters packed into one integer): (first positions (s, i), counts) in output order"""
    assert k <= 8
    keys, where = [], []
    for s, x in enumerate(strings):
        a = np.frombuffer(x, np.uint8).astype(np.uint64)
        if len(a) < k:
            continue
        n = len(a) - k + 1
        key = np.zeros(n, np.uint64)
        ok = np.ones(n, bool)
        for j in range(k):
            key = (key << np.uint64(8)) | a[j:j + n]
            ok &= a[j:j + n] != gap[0]
        idx = np.nonzero(ok)[0]
        keys.append(key[idx])
        where.append(np.stack([np.full(len(idx), s, np.int64), idx.astype(np.int64)], 1))
    if not keys:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    keys, where = np.concatenate(keys), np.concatenate(where)
    _, first, counts = np.unique(keys, return_index=True, return_counts=True)
    keep = counts >= min_mult
    first, counts = first[keep], counts[keep]
    order = np.argsort(first, kind="stable")
    return where[first[order]], counts[order]


def check_np(eng, strings, k, min_mult, n_distinct_above=0):
    where, counts = restate_np(strings, k, min_mult)
    first, ptr, occ = eng.monokmers(strings, k, min_mult, True)
    assert np.array_equal(first["s"], where[:, 0]) and np.array_equal(first["i"], where[:, 1]) and np.array_equal(first["count"], counts)
    assert np.array_equal(np.diff(ptr), counts) and ptr[-1] == len(occ)
    # every occurrence list ascends in (s, i), starts at the first occurrence and holds the k-mer's letters
    key = occ["s"].astype(np.int64) << 32 | occ["i"].astype(np.int64)
    inner = np.ones(len(occ), bool)
    inner[ptr[:-1]] = False
    assert np.all(np.diff(key)[inner[1:]] > 0)
    assert np.array_equal(occ["s"][ptr[:-1]], first["s"]) and np.array_equal(occ["i"][ptr[:-1]], first["i"])
    flat = np.frombuffer(b"".join(strings), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in strings])])
    owner = np.repeat(np.arange(len(first)), counts)
    for j in range(k):
        assert np.array_equal(flat[off[occ["s"]] + occ["i"] + j], flat[first["pos"][owner] + j])
    assert eng.monokmers_info()["n_distinct"] > n_distinct_above
    return first

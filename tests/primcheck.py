"""The primitives of cf_prims.hip that every stage stands on, one call each, against numpy: the stable sort of 16-byte records
(cf_radix_sort_rec16 = cf_rec16_hist, the scan of its digit-major histogram, cf_rec16_scatter), the scan of 32-bit counts into
64-bit offsets and the 64-bit scan through all three levels of its recursion, out of place and in place, and the offsets of
tile-major digit histograms (cf_tile_digit_offsets = cf_col_sum_kernel, cf_col_base_kernel, cf_col_offs_kernel).  The stages
reach them only with the digit patterns, widths and sizes their own inputs happen to make; here every case is built around a
border of the kernels: the tile of 2048 records, the wave of 64 lanes inside a round of 256, the invalid lanes of a partial last
round (their zeroed record has digit 0), the scan's tile of 2048 and its square, the 512 threads and the chunks of 16, 32, 48
tiles of the column walk.

The tiles come from the library (Engine.monokmers_info: sort_tile, scan_tile); check_tiles pins them to the figures the sizes
below were chosen around, so a changed tile fails there and not silently somewhere else.  A size is written (tiles, extra).
Every record carries its input index (or a hash of it) in each word that is not a sort field, and whole records are compared:
a lost, doubled or torn record and any breach of stability differ from the reference.  All comparisons are integer-exact.
Used by test_emu_prims.py (host emulator) and test_gpu_prims.py (MI355X)."""
import numpy as np

from centroflye_amd.engine import DeviceError

WAVE = 64                     # lanes of a wave; four waves make a round of cf_rec16_scatter
SCAN_ITEMS = 8                # items per thread of cf_scan_local
COL_THREADS, COL_UNROLL = 512, 16      # cf_tile_digit_offsets: a thread per digit; its chunks are multiples of 16 tiles


def tiles(engine):
    info = engine.monokmers_info()
    return info["sort_tile"], info["scan_tile"]


def size_id(size):
    """(tiles, extra) or (tiles squared, tiles, extra) as a test id"""
    return "+".join(f"{c}{u}" for c, u in zip(size, ("t2", "t", "") if len(size) == 3 else ("t", "")) if c or not u)


def check_tiles(engine):
    """The borders the cases are built around: a tile of the record sort is 8 rounds of 4 waves, a tile of the scan 256 threads of
    8 items, and the sizes called `third level` are beyond the square of the scan's tile."""
    sort_tile, scan_tile = tiles(engine)
    assert sort_tile == 2048 and sort_tile % (4 * WAVE) == 0
    assert scan_tile == 2048 and scan_tile % SCAN_ITEMS == 0
    assert scan_size(engine, (1, 0, 1)) == 2048 * 2048 + 1 and scan_size(engine, (2, 1, 3)) == 2 * 2048 * 2048 + 2048 + 3


# ------------------------------------------------------------------ the record sort
def _hash(i):
    x = (i.astype(np.uint64) + np.uint64(0x9E3779B9)) * np.uint64(0x85EBCA6B) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return (x * np.uint64(0xC2B2AE35) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def records(n, fields):
    """n records; fields: {word: uint32 array}.  Of the other words the first holds the input index, the rest a hash of it."""
    recs = np.zeros((n, 4), np.uint32)
    idx = np.arange(n, dtype=np.uint32)
    first = True
    for w in range(4):
        if w in fields:
            recs[:, w] = fields[w]
        else:
            recs[:, w] = idx if first else _hash(idx + np.uint32(w))
            first = False
    assert not first, "no word left for the input index"
    return recs


def sorted_bits(bits):
    return (bits + 7) // 8 * 8


def reference_sort(recs, words, bits):
    """np.lexsort (stable; its last key is the most significant one, as the field list's) on the fields masked to whole bytes."""
    keys = [recs[:, w] & np.uint32((1 << sorted_bits(b)) - 1) for w, b in zip(words, bits) if b > 0]
    return recs[np.lexsort(keys)] if keys and recs.shape[0] else recs.copy()


def check_sort(engine, recs, words, bits, what=""):
    got = engine.selftest_sort_rec16(recs, words, bits)
    want = reference_sort(recs, words, bits)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {recs.shape[0]} records differ from the stable reference, the first at {bad[0]}: "
                             f"{got[bad[0]].tolist()} for {want[bad[0]].tolist()}")
    return got


def sort_size(engine, size):
    return size[0] * tiles(engine)[0] + size[1]


SORT_SIZES = [(0, 0), (0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (0, 255), (0, 256), (0, 257), (1, -1), (1, 0), (1, 1), (3, 77)]


def sort_sizes(engine, size):
    """One field of 8 bits, taken from each of the four words in turn (the word's other three bytes hold random bits that take no
    part)."""
    n = sort_size(engine, size)
    rng = np.random.default_rng(1000 + n)
    for word in range(4):
        key = rng.integers(0, 256, n, dtype=np.uint32)
        check_sort(engine, records(n, {word: key | (rng.integers(0, 2 ** 24, n, dtype=np.uint32) << np.uint32(8))}), [word], [8], f"n={n} word {word}")


def _digit_cases(engine):
    """(name, n, digits): the digit of every record, laid out by the waves of the scatter (record i of a tile is lane i % 64 of
    wave (i / 64) % 4 in round i / 256)."""
    tile = tiles(engine)[0]
    rng = np.random.default_rng(64)
    n = 2 * tile + 3 * WAVE + 5
    i = np.arange(n)
    yield "every wave one digit", n, _hash((i // WAVE).astype(np.uint32)) & np.uint32(255)
    yield "every wave one digit, a round's waves the same", n, _hash((i // (4 * WAVE)).astype(np.uint32)) & np.uint32(255)
    distinct = np.concatenate([rng.permutation(256)[:WAVE] for _ in range((n + WAVE - 1) // WAVE)])[:n]
    assert all(np.unique(distinct[j:j + WAVE]).size == min(WAVE, n - j) for j in range(0, n, WAVE))
    yield "64 distinct digits in every wave", n, distinct
    yield "digits 0 and 255 only", n, rng.integers(0, 2, n) * 255
    for b in range(8):
        x = int(rng.integers(0, 256))
        yield f"digits {x} and {x ^ (1 << b)} (bit {b} apart)", n, np.where(rng.integers(0, 2, n) == 1, x, x ^ (1 << b))
    yield "every digit 0, the last round partial", tile + 37, np.zeros(tile + 37, np.int64)
    yield "every digit 0 but the last wave's, the last round partial", tile + 37, np.where(i[:tile + 37] >= tile, 1 + i[:tile + 37] % 3, 0)


def sort_wave_patterns(engine):
    """The patterns as the lowest byte of a one-pass sort and as the highest byte of a four-pass one (the three passes below it
    see a single digit, 0)."""
    names = []
    for name, n, digit in _digit_cases(engine):
        digit = np.asarray(digit, np.uint32)
        assert digit.size == n and int(digit.max(initial=0)) < 256
        check_sort(engine, records(n, {1: digit}), [1], [8], name)
        check_sort(engine, records(n, {2: digit << np.uint32(24)}), [2], [32], name + " (byte 3)")
        names.append(name)
    assert len(names) == 14
    return names


def sort_stability(engine):
    tile = tiles(engine)[0]
    n = 2 * tile + 77
    recs = records(n, {0: np.full(n, 0xA5A5A5A5, np.uint32), 3: np.full(n, 7, np.uint32)})
    got = check_sort(engine, recs, [3, 0], [32, 32], "all keys equal")
    assert np.array_equal(got, recs), "all keys equal: the output is not the input"
    rng = np.random.default_rng(5)
    n = 5 * tile + 3
    key = np.where(rng.random(n) < 0.9, 7, rng.integers(0, 1 << 16, n)).astype(np.uint32)
    assert (key == 7).sum() > 0.85 * n
    got = check_sort(engine, records(n, {2: key}), [2], [16], "90 % on one digit")
    assert np.array_equal(got[:, 0][got[:, 2] == 7], np.flatnonzero(key == 7)), "the records of the heavy digit left their input order"
    # runs of one digit longer than a tile: whole tiles whose histogram has one entry
    key[tile // 2: 2 * tile + tile // 2 + 9] = 7
    check_sort(engine, records(n, {2: key}), [2], [16], "a run of one digit over more than two tiles")


def sort_pass_parity(engine):
    """1 and 3 passes end in the scratch buffer (the copy back must happen), 2 and 4 in place; bits = 0 is no pass at all."""
    tile = tiles(engine)[0]
    n = tile + 300
    rng = np.random.default_rng(11)
    key = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    for bits in (0, 8, 16, 24, 32):
        recs = records(n, {1: key & np.uint32((1 << bits) - 1)})
        got = check_sort(engine, recs, [1], [bits], f"{bits // 8} passes")
        assert (bits == 0) == np.array_equal(got, recs)
    recs = records(n, {1: key & np.uint32(0xFF), 2: key >> np.uint32(24)})
    check_sort(engine, recs, [1, 2], [8, 8], "two fields of one pass")
    check_sort(engine, recs, [1, 2, 0], [8, 0, 0], "one pass and two empty fields")
    assert np.array_equal(engine.selftest_sort_rec16(recs, [], []), recs)


MONO_BITS = (1, 8, 9, 16, 17, 24, 32)


def sort_monokmer_fields(engine, b):
    """{1, 0} with (b, b): a round of the mono-k-mer counter's prefix doubling (cf_monokmers.hip), ids below 2^b; and its first
    round, word 0 alone."""
    tile = tiles(engine)[0]
    n = 2 * tile + 5
    rng = np.random.default_rng(200 + b)
    hi = min(2 ** b, n)                     # ids are ranks: fewer than records, so equal pairs meet and stability shows
    recs = records(n, {0: rng.integers(0, hi, n, dtype=np.uint32), 1: rng.integers(0, hi, n, dtype=np.uint32)})
    assert int(recs[:, :2].max()) < 2 ** b
    check_sort(engine, recs, [1, 0], [b, b], f"mono-k-mer round, {b} bits")
    check_sort(engine, recs, [0], [b], f"mono-k-mer first round, {b} bits")


def sort_edge_fields(engine, kbits):
    """{2, 1, 0} with (kbits, kbits, 16): cf_sort_edges — rows (d, a, b, freq) by d, then a, then b."""
    tile = tiles(engine)[0]
    n = tile + 700
    rng = np.random.default_rng(300 + kbits)
    few = min(2 ** kbits, 40)               # few first k-mers: every (d, a) has several b
    recs = records(n, {0: rng.integers(1, 5, n, dtype=np.uint32) * np.uint32(16383), 1: rng.integers(0, few, n, dtype=np.uint32) * np.uint32((2 ** kbits - 1) // max(few - 1, 1)),
                       2: rng.integers(0, 2 ** kbits, n, dtype=np.uint32)})
    assert int(recs[:, 0].max()) < 2 ** 16 and int(recs[:, 1:3].max()) < 2 ** kbits
    check_sort(engine, recs, [2, 1, 0], [kbits, kbits, 16], f"edge rows, {kbits} bits")


def sort_tandem_fields(engine, nb):
    """{0, 1, 2} with (32, 30, bits of nb): the tandem scan's 16-byte records at k = 31 (62 code bits, then the read in the batch;
    the value nb marks an invalid record)."""
    tile = tiles(engine)[0]
    n = tile + 300
    rng = np.random.default_rng(400 + nb)
    bits_nb = max(1, int(nb).bit_length())
    codes = rng.integers(0, 2 ** 62, 50, dtype=np.uint64)[rng.integers(0, 50, n)]      # repeated codes: a read's runs
    recs = records(n, {0: (codes & np.uint64(0xFFFFFFFF)).astype(np.uint32), 1: (codes >> np.uint64(32)).astype(np.uint32),
                       2: rng.integers(0, nb + 1, n, dtype=np.uint32)})
    assert int(recs[:, 1].max()) < 2 ** 30 and int(recs[:, 2].max()) == nb < 2 ** bits_nb
    check_sort(engine, recs, [0, 1, 2], [32, 30, bits_nb], f"tandem records, {nb} reads in the batch")


def sort_bits_contract(engine):
    """bits = 5 sorts the low byte.  (a) bits 8 .. 31 of the word take no part: records equal in the low byte keep their input
    order whatever is above it.  (b) bits 5 .. 7 take part: the output is ordered by the whole byte, not by five bits."""
    tile = tiles(engine)[0]
    n = tile + 500
    rng = np.random.default_rng(55)
    low = rng.integers(0, 32, n, dtype=np.uint32)
    junk = rng.integers(0, 2 ** 24, n, dtype=np.uint32) << np.uint32(8)
    got = check_sort(engine, records(n, {0: low | junk}), [0], [5], "bits above the rounded width")
    plain = check_sort(engine, records(n, {0: low}), [0], [5], "no bits above the width")
    assert np.array_equal(got[:, 1], plain[:, 1]), "bits above the rounded width changed the order"
    key = got[:, 0] & np.uint32(0xFF)
    assert (np.diff(key.astype(np.int64)) >= 0).all() and (np.diff(got[:, 1].astype(np.int64))[np.diff(key.astype(np.int64)) == 0] > 0).all()
    assert (np.diff(got[:, 0].astype(np.int64)) < 0).any()          # (the case: the whole word is NOT in order)
    byte = rng.integers(0, 256, n, dtype=np.uint32)
    recs = records(n, {0: byte})
    got = check_sort(engine, recs, [0], [5], "bits between the width and the byte border")
    assert (np.diff(got[:, 0].astype(np.int64)) >= 0).all()
    five = recs[np.argsort(byte & np.uint32(31), kind="stable")]
    assert not np.array_equal(got, five), "the case cannot tell a five-bit sort from a byte sort"


def sort_many_tiles(engine, n_tiles=2049):
    """n_tiles tiles and 5 records, two fields of 13 bits: the histogram is 256 x n_tiles counters, its scan has more than one
    block (more than a scan tile of them from 9 tiles on; 2049 tiles: 257 blocks and the second level)."""
    tile, scan_tile = tiles(engine)
    assert 256 * n_tiles > scan_tile
    n = n_tiles * tile + 5
    rng = np.random.default_rng(9)
    recs = records(n, {0: rng.integers(0, 2 ** 13, n, dtype=np.uint32), 1: rng.integers(0, 2 ** 13, n, dtype=np.uint32)})
    check_sort(engine, recs, [0, 1], [13, 13], f"{n_tiles} tiles")


# ------------------------------------------------------------------ the scans
SCAN_SMALL = [(0, 0, 0), (0, 0, 1), (0, 0, 7), (0, 0, 8), (0, 0, 9), (0, 1, -1), (0, 1, 0), (0, 1, 1)]
SCAN_SQUARE = [(1, 0, -1), (1, 0, 0), (1, 0, 1)]           # around the square of the tile: where the third level begins
SCAN_THIRD = [(1, 0, 1), (2, 1, 3)]


def scan_size(engine, size):
    t = tiles(engine)[1]
    return size[0] * t * t + size[1] * t + size[2]


def reference_scan(v):
    out = np.zeros(v.size + 1, np.int64)
    np.cumsum(v, dtype=np.int64, out=out[1:])
    return out


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, the first at {bad[0]}: {int(got[bad[0]])} for {int(want[bad[0]])}")


def scan_u32(engine, size):
    """cf_scan_exclusive_u32_to_i64: all 0xFFFFFFFF (the eight items of one thread already pass 2^32), all 0, all 1 and random
    counts over the full range."""
    n = scan_size(engine, size)
    rng = np.random.default_rng(n)
    for name, v in (("all 0xFFFFFFFF", np.full(n, 0xFFFFFFFF, np.uint32)), ("all 0", np.zeros(n, np.uint32)), ("all 1", np.ones(n, np.uint32)),
                    ("random", rng.integers(0, 2 ** 32, n, dtype=np.uint32))):
        want = reference_scan(v)
        if name == "all 0xFFFFFFFF":
            assert int(want[-1]) == n * 0xFFFFFFFF and (n < SCAN_ITEMS or int(want[SCAN_ITEMS]) >= 2 ** 32)
        _same(engine.selftest_scan_u32(v), want, f"u32 scan of {n}, {name}")


def scan_i64_and_inplace(engine, size):
    """Values in [2^39, 2^40) through cf_scan_exclusive_i64 with two buffers and with one: the same array, the reference's."""
    n = scan_size(engine, size)
    v = np.random.default_rng(n).integers(2 ** 39, 2 ** 40, n, dtype=np.int64)
    assert float(v.sum(dtype=np.float64)) < 0.9 * 2.0 ** 63          # the sums stay inside 64 bits
    want = reference_scan(v)
    apart = engine.selftest_scan(v)
    _same(apart, want, f"i64 scan of {n}")
    inplace = engine.selftest_scan_inplace(v)
    _same(inplace, apart, f"i64 scan of {n} in place against out of place")


# ------------------------------------------------------------------ the offsets of tile-major digit histograms
DIGITS = (1, 2, 63, 64, 65, 255, 256, 257, 512)
DIGITS_CROSSED = (1, 65, 256, 512)
TILE_COUNTS = (1, 15, 16, 17, 255, 256, 257, 1025)
TILE_COUNTS_FEW = (17, 257)


def col_chunk(n_tiles):
    """cf_prims.hip: tiles per chunk of the column walk — the first multiple of 16 whose square reaches n_tiles."""
    c = COL_UNROLL
    while c * c < n_tiles:
        c += COL_UNROLL
    return c


def reference_offsets(hist):
    flat = hist.T.astype(np.int64).ravel()
    ex = np.zeros(flat.size + 1, np.int64)
    np.cumsum(flat, out=ex[1:])
    return ex[:-1].reshape(hist.shape[1], hist.shape[0]).T, int(ex[-1])


def check_offsets(engine, hist, what):
    n_tiles, D = hist.shape
    # the bound the kernels stand on: a chunk's column sum is a 32-bit counter
    chunk = col_chunk(n_tiles)
    assert int(np.add.reduceat(hist.astype(np.int64), np.arange(0, n_tiles, chunk), axis=0).max()) < 2 ** 32, what
    want, total = reference_offsets(hist)
    for with_total in (True, False):
        offs, got_total = engine.selftest_digit_offsets(hist, n_tiles, D, with_total=with_total)
        _same(offs.ravel(), want.ravel(), f"{what}, offsets ({'with' if with_total else 'no'} total)")
        assert got_total == (total if with_total else None), f"{what}: total {got_total} for {total}"
    return total


def digit_offsets(engine, D):
    assert [col_chunk(t) for t in (1, 16, 17, 256, 257, 1024, 1025)] == [16, 16, 16, 16, 32, 32, 48]
    largest = 0
    for n_tiles in (TILE_COUNTS if D in DIGITS_CROSSED else TILE_COUNTS_FEW):
        rng = np.random.default_rng(10000 * D + n_tiles)
        hist = rng.integers(0, 65537, (n_tiles, D), dtype=np.uint32)
        largest = max(largest, check_offsets(engine, hist, f"D={D}, {n_tiles} tiles"))
    if D == max(DIGITS):
        assert largest >= 2 ** 32, "the largest shape was to pass 32 bits in the total"
    return largest


def digit_offsets_special_counts(engine):
    for D, n_tiles in ((65, 257), (512, 33), (256, 1025)):
        assert check_offsets(engine, np.zeros((n_tiles, D), np.uint32), f"all zero, D={D}") == 0
        for d in sorted({0, D // 2, D - 1}):
            hist = np.zeros((n_tiles, D), np.uint32)
            hist[:, d] = np.random.default_rng(d).integers(1, 65537, n_tiles, dtype=np.uint32)
            check_offsets(engine, hist, f"digit {d} of {D} holds everything")


def digit_offsets_refusals(engine):
    """D = 0 and D = 513 are refused (-22) and the context works afterwards; no tiles: 0, and nothing is written."""
    for D in (0, COL_THREADS + 1):
        try:
            engine.selftest_digit_offsets(np.ones(4 * max(D, 1), np.uint32), 4, D)
        except DeviceError as e:
            assert "(-22)" in str(e) and "digit count" in str(e), str(e)
        else:
            raise AssertionError(f"D = {D} was accepted")
        check_offsets(engine, np.arange(3 * 5, dtype=np.uint32).reshape(3, 5), "after a refusal")
    for D in (1, 256, COL_THREADS):
        for with_total in (True, False):
            offs, total = engine.selftest_digit_offsets(np.zeros(0, np.uint32), 0, D, with_total=with_total, fill=-77)
            assert offs.size == 0 and total == (-77 if with_total else None), "no tiles: the total was written"

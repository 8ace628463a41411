"""The generic LSD radix sort of 64-bit keys (cf_prims.hip: tile-major digit counts, LDS-staged stable scatter) on the
host emulator: tiles of 4096 keys cut at and across their boundaries, a grid that strides over more tiles than it has
workgroups, key widths that are not a multiple of the 8-bit digit, and stability — the bits above the sorted bytes are a
payload that must keep its input order inside every key (the postings sort keeps units ascending within a k-mer)."""
import numpy as np
import pytest

from centroflye_amd.engine import Engine

TILE = 4096


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def _stable(keys, bits):
    sorted_bits = (bits + 7) // 8 * 8
    low = keys & np.uint64((1 << sorted_bits) - 1) if sorted_bits < 64 else keys
    return keys[np.argsort(low, kind="stable")]


@pytest.mark.parametrize("n", [2, TILE - 1, TILE, TILE + 1, 3 * TILE + 77])
def test_sort_across_tile_boundaries(engine, n):
    rng = np.random.default_rng(n)
    k = rng.integers(0, 2 ** 24, n, dtype=np.uint64)
    assert np.array_equal(engine.selftest_sort(k, 24), np.sort(k))


@pytest.mark.parametrize("bits", [6, 13, 38])
def test_stable_on_widths_not_a_multiple_of_the_digit(engine, bits):
    rng = np.random.default_rng(bits)
    n = 2 * TILE + 999
    sorted_bits = (bits + 7) // 8 * 8
    key = rng.integers(0, 2 ** bits, n, dtype=np.uint64)
    payload = np.arange(n, dtype=np.uint64) % np.uint64(1 << (62 - sorted_bits))     # ascending: the input order
    k = key | (payload << np.uint64(sorted_bits))
    got = engine.selftest_sort(k, bits)
    assert np.array_equal(got, _stable(k, bits))


def test_skewed_digits_and_runs_longer_than_a_tile(engine):
    rng = np.random.default_rng(5)
    n = 5 * TILE + 3
    key = np.where(rng.random(n) < 0.9, 7, rng.integers(0, 1 << 16, n)).astype(np.uint64)      # one digit fills whole tiles
    k = key | (np.arange(n, dtype=np.uint64) << np.uint64(16))
    assert np.array_equal(engine.selftest_sort(k, 16), _stable(k, 16))


def test_grid_strides_over_more_tiles_than_workgroups(engine):
    # the grid is at most 8 workgroups per CU: the emulated device's 4 CUs stride over 40 tiles
    rng = np.random.default_rng(9)
    n = 40 * TILE + 5
    k = rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64)
    assert np.array_equal(engine.selftest_sort(k, 64), np.sort(k))

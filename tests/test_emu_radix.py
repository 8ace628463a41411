"""The generic LSD radix sort of 64-bit keys (cf_prims.hip: tile-major digit counts, LDS-staged stable scatter) on the
host emulator: tiles of 4096 keys cut at and across their boundaries, a grid that strides over more tiles than it has
workgroups, key widths that are not a multiple of the 8-bit digit, and stability — the bits above the sorted bytes are a
payload that must keep its input order inside every key (the postings sort keeps units ascending within a k-mer).  The bodies
live in tests/shapecheck.py: tests/test_gpu_shapes.py runs them on an MI355X, with a size that makes the real grid stride."""
import pytest

import shapecheck
from centroflye_amd.engine import Engine

TILE = shapecheck.TILE


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


@pytest.mark.parametrize("n", [2, TILE - 1, TILE, TILE + 1, 3 * TILE + 77])
def test_sort_across_tile_boundaries(engine, n):
    shapecheck.radix_across_tile_boundaries(engine, n)


@pytest.mark.parametrize("bits", [6, 13, 38])
def test_stable_on_widths_not_a_multiple_of_the_digit(engine, bits):
    shapecheck.radix_stable_on_odd_widths(engine, bits)


def test_skewed_digits_and_runs_longer_than_a_tile(engine):
    shapecheck.radix_skewed_digits(engine)


def test_grid_strides_over_more_tiles_than_workgroups(engine):
    # the grid is at most 8 workgroups per CU: the emulated device's 4 CUs stride over 40 tiles
    shapecheck.radix_grid_strides(engine, 40)
    shapecheck.scan_of_wide_values(engine, 100003)

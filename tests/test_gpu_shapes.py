"""-m gpu: the shape cases of tests/shapecheck.py on a real MI355X — all four families in full, family 1 once more under
lut_shift 0 and 3, family 2 under count_tile 1 / 64 and count_slots 256, and the generic radix sort and scan on a grid that
really strides (2049 tiles on 2048 workgroups).  cf_cloud_kernel's sort and compaction are made of ballots, readfirstlane, LDS
atomics and barriers, A1's first pass of byte-aligned word loads and a 128-bit shift: the host emulator (test_emu_shapes.py)
cannot show a wave-level mistake in them, and the generator-made inputs of the other GPU tests stay inside one regime of each.
Integer-exact throughout; every case asserts its regime from the plain reference before the device runs."""
import pytest

import shapecheck
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


# ------------------------------------------------------------------ family 1: cloud size regimes
@pytest.mark.parametrize("lut_shift", [-1, 0, 3])
def test_cloud_size_regimes(engine, lut_shift):
    """Counting rank (<= 512), bitonic network in the 2048-slot set (<= 1536), the 8192-slot retry (<= 6144), the refusal at
    6145 with the context usable afterwards, a launch whose retry repeats units that had fitted, the staging-tile borders."""
    with engine.knobs(lut_shift=lut_shift):
        for n in shapecheck.CLOUD_SIZES:
            shapecheck.check_shapes(engine, shapecheck.cloud_size_case(n))
        shapecheck.check_shapes(engine, shapecheck.cloud_size_case(6145))
        shapecheck.check_shapes(engine, shapecheck.cloud_size_case(1536))
        shapecheck.check_shapes(engine, shapecheck.cloud_mixed_case())
        shapecheck.check_shapes(engine, shapecheck.cloud_staging_case())


# ------------------------------------------------------------------ family 2: A1's first pass
TABLE_KNOBS = (dict(), dict(count_tile=1), dict(count_tile=64), dict(count_slots=256))


@pytest.mark.parametrize("k", shapecheck.A1_KS)
def test_a1_lengths_alignments_and_symbols(engine, k):
    """Every read set through A1 -> A6 with sort and reduce (k = 30, 31: the table path by itself), then A1 and A2 on the
    atomic table with its default tiles, tiles of 1 and of 64 windows per thread, and LDS sets of 256 slots."""
    for e in range(4):
        for symbols in (0, 1):
            case = shapecheck.a1_case(k, e, symbols)
            shapecheck.check_shapes(engine, case)
            for knobs in TABLE_KNOBS:
                with engine.knobs(count_mode=0, **knobs):
                    shapecheck.check_shapes(engine, case, upto="A2")


# ------------------------------------------------------------------ family 3: few reads, repeats
@pytest.mark.parametrize("k", [4, 11, 19, 25])
@pytest.mark.parametrize("R", [1, 2, 3, 5])
def test_few_reads_with_repeats(engine, R, k):
    """One read is the record without read bits; a 600-base stretch twice in every read and in all of them: the
    multi-occurrence cut at max_nonuniq 0, 1, 2; occurrence counts and top n with ties at the cut, on both A1 paths."""
    for max_nonuniq in (0, 1, 2):
        case = shapecheck.repeats_case(R, k, max_nonuniq)
        shapecheck.check_shapes(engine, case)
        with engine.knobs(count_mode=0):
            shapecheck.check_shapes(engine, case, upto="A2")
    reads = shapecheck.repeats_case(R, k, 0)["reads"]
    shapecheck.check_occurrences(engine, reads, k)
    with engine.knobs(count_mode=0):
        shapecheck.check_occurrences(engine, reads, k)


# ------------------------------------------------------------------ family 4: dense clouds through the distance stage
@pytest.mark.parametrize("name", list(shapecheck.DENSE))
def test_dense_clouds(engine, name):
    shapecheck.check_dense(engine, name)


def test_dense_clouds_spill_under_a_small_table(engine):
    """The first dense case with 512 slots and every (b, d) pair in the exact table: first k-mers whose table has to be
    partitioned (n_spilled > 0)."""
    with engine.knobs(dist_slots=512, dist_sketch=0):
        shapecheck.check_dense(engine, "dense_2x5")
        assert engine.stats()["n_spilled"] > 0


# ------------------------------------------------------------------ the generic radix sort and scan
def test_radix_sort_bodies_of_the_emulator_suite(engine):
    for n in (2, shapecheck.TILE - 1, shapecheck.TILE, shapecheck.TILE + 1, 3 * shapecheck.TILE + 77):
        shapecheck.radix_across_tile_boundaries(engine, n)
    for bits in (6, 13, 38):
        shapecheck.radix_stable_on_odd_widths(engine, bits)
    shapecheck.radix_skewed_digits(engine)
    shapecheck.radix_grid_strides(engine, 40)


def test_radix_sort_grid_strides_on_the_real_device(engine):
    """min(tiles, 8 x 256 CUs) = 2048 workgroups: 2049 tiles and 5 keys make one workgroup take a second tile, the last one
    partial.  64-bit keys, and 13-bit keys whose payload (the input index) must keep its order."""
    assert engine.device_info()["n_cu"] * 8 < 2049
    shapecheck.radix_grid_strides(engine, 2049)


@pytest.mark.parametrize("n", [100003, 3_000_001])
def test_scan_of_values_beyond_32_bits(engine, n):
    shapecheck.scan_of_wide_values(engine, n)

"""-m gpu: the distance kernel's sketch, bitmap and table split with their collisions planted (tests/collidecheck.py) on a real MI355X,
in the launch shapes the library picks by itself and under one wave.  Here the 16 adds of a wave step reach a 4-bit counter before
any of them is taken back (the host emulator of test_emu_dist_collisions.py never wraps one), the waves of the default workgroup
interleave their adds, and a set of 2^24 + 6 k-mers is affordable: the sketch collision of the region layouts."""
import pytest

import collidecheck as col
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("min_cov, n, k", col.FOUR_BIT)
def test_a_victim_shares_a_4_bit_counter_with_a_burst_of_16(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k)


@pytest.mark.parametrize("min_cov, n, k", col.BYTES)
def test_a_victim_shares_a_byte_counter_with_a_burst_that_wraps_it(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k)


@pytest.mark.parametrize("min_cov, n, k", col.BYTES_AT_9)
def test_a_victim_shares_a_byte_counter_at_min_cov_9(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, extra=dict(dist_sketch_bits=8))


@pytest.mark.parametrize("min_cov, n, k", col.BOTH)
def test_a_burst_wraps_the_4_bit_counter_and_then_the_byte(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k)


@pytest.mark.parametrize("min_cov, n, k", (col.FOUR_BIT[1], col.BYTES[0], col.BOTH[0]))
def test_victims_one_short_of_min_cov_are_not_selected(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, short=True)


@pytest.mark.parametrize("several", (False, True))
@pytest.mark.parametrize("min_cov", col.F2_MIN_COVS)
def test_ranks_that_share_a_bitmap_bit(engine, min_cov, several):
    col.run_aliases(engine, min_cov, several)


@pytest.mark.parametrize("min_cov, n, k", ((9, 16, 4), (10, 255, 5)))
def test_ranks_2_to_the_24_apart_share_a_sketch_counter_in_the_region_layouts(engine, min_cov, n, k):
    col.run_region_collision(engine, min_cov, n, k)


@pytest.mark.parametrize("sketch", (1, 0))
@pytest.mark.parametrize("layout", list(col.F3_LAYOUTS))
def test_a_partner_that_cannot_be_split_away_is_refused_not_lost(engine, layout, sketch):
    col.run_unsplittable(engine, layout, sketch)

"""The distance kernel's sketch, bitmap and table split with their collisions planted (tests/collidecheck.py), on the host-emulated
kernels.  tests/test_gpu_dist_collisions.py runs the same cases on an MI355X, and the ones that need a device:
  - the emulator runs the lanes of a wave one after the other, so a lane's take-backs come before the next lane's adds and a 4-bit
    counter never passes 15 here: the bursts of 16 raise the wrap flag (a lane sees 12 .. 15) and the sweep runs again with bytes, but
    the victim would survive without either.  On a device the 16 adds of the step come before any take-back, the field is left at 0
    and only the flag saves the victim.  The byte cases wrap here as they do there;
  - the sketch collision of the region layouts needs a set of 2^24 + 6 k-mers;
  - the layouts of family 1 run here with the bursts of 16 alone, the bursts of 254 and 255 under one wave (a launch of their 180 000
    cloud entries outside the groups takes the emulator ten seconds and more), and family 3 in four of its six settings."""
import pytest

import collidecheck as col
from centroflye_amd.engine import Engine

BASE = dict(dist_block=128)      # (where a setting leaves the workgroup to the library: the emulator's time per launch goes with its threads)
ONE_WAVE = {k: col.F1_SETTINGS[k] for k in ("one_wave", "one_wave_small_table")}
CONTROL = {k: col.F1_SETTINGS[k] for k in ("one_wave", "one_wave_small_table", "no_sketch")}      # (without the sketch every partner entry goes through the table: 64 passes)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
    yield e
    e.close()


@pytest.mark.parametrize("min_cov, n, k", col.FOUR_BIT)
def test_a_victim_shares_a_4_bit_counter_with_a_burst_of_16(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, CONTROL)


@pytest.mark.parametrize("min_cov, n, k", col.BYTES)
def test_a_victim_shares_a_byte_counter_with_a_burst_that_wraps_it(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, CONTROL if (min_cov, n, k) == col.BYTES[0] else ONE_WAVE)


@pytest.mark.parametrize("min_cov, n, k", col.BYTES_AT_9)
def test_a_victim_shares_a_byte_counter_at_min_cov_9(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, ONE_WAVE, dict(dist_sketch_bits=8))


@pytest.mark.parametrize("min_cov, n, k", col.BOTH)
def test_a_burst_wraps_the_4_bit_counter_and_then_the_byte(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, ONE_WAVE)


@pytest.mark.parametrize("min_cov, n, k", (col.FOUR_BIT[1],))
def test_victims_and_bursts_in_every_layout(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, {k_: v for k_, v in col.F1_SETTINGS.items() if k_ not in CONTROL})


@pytest.mark.parametrize("min_cov, n, k", (col.FOUR_BIT[1], col.BYTES[0], col.BOTH[0]))
def test_victims_one_short_of_min_cov_are_not_selected(engine, min_cov, n, k):
    col.run_victims(engine, min_cov, n, k, ONE_WAVE, short=True)


@pytest.mark.parametrize("several", (False, True))
@pytest.mark.parametrize("min_cov", col.F2_MIN_COVS)
def test_ranks_that_share_a_bitmap_bit(engine, min_cov, several):
    col.run_aliases(engine, min_cov, several)


@pytest.mark.parametrize("layout, sketch", (("default", 1), ("narrow", 1), ("wide", 1), ("narrow", 0)))
def test_a_partner_that_cannot_be_split_away_is_refused_not_lost(engine, layout, sketch):
    col.run_unsplittable(engine, layout, sketch)

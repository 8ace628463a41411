"""-m gpu: the distance stage where a pair's count meets a border — min_cov against the counting sketch's switches (2, 10, 200), counts
against the ranges of its counters (12, 15, 255) and against the 15-bit count fields of the exact table (32767) — on a real MI355X: the
cases of tests/countcheck.py, every one of which selects edges, against the oracle, in the launch shapes the library picks by itself.
Here the sketch's adds of different waves interleave (the host emulator of test_emu_dist_counts.py runs them one after the other),
and every layout of the posting-list border runs."""
import pytest

import countcheck as cc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("min_cov", cc.MIN_COVS)
def test_counts_one_short_of_min_cov_at_it_and_one_above(engine, min_cov):
    cc.run_around(engine, min_cov)


@pytest.mark.parametrize("min_cov", cc.MIN_COVS)
def test_counts_around_min_cov_in_a_table_that_splits_and_a_filter_inside_the_scan(engine, min_cov):
    cc.run_around(engine, min_cov, cc.PRESSURE)


@pytest.mark.parametrize("min_cov", cc.RANGE_MIN_COVS)
def test_counts_past_15_and_255_are_selected_with_their_exact_count(engine, min_cov):
    cc.run_range(engine, min_cov)


@pytest.mark.parametrize("min_cov", cc.RANGE_MIN_COVS)
def test_counts_past_15_and_255_when_every_b_marked_sets_up_partitions(engine, min_cov):
    cc.run_range(engine, min_cov, cc.PRESSURE)
    if min_cov <= 9:      # (from 10 on the counters are bytes anyway)
        cc.run_range(engine, min_cov, cc.PRESSURE, dict(dist_sketch_bits=8))


@pytest.mark.parametrize("min_cov", cc.BURST_MIN_COVS)
@pytest.mark.parametrize("n", cc.BURSTS)
def test_a_burst_of_adds_on_one_counter_out_of_one_item(engine, n, min_cov):
    """One posting whose partner unit holds one rank n times: the adds of one wave step, four per lane, all issued before any of them
    is taken back — 16 and more wrap a 4-bit counter (the first k-mer is swept again with bytes), 256 and more a byte ("every b
    marked"): test_emu_dist_counts.py says what was seen of it on the emulator."""
    cc.run_burst(engine, n, min_cov)


def test_the_histogram_written_down_for_the_posting_lists_is_the_oracles(engine):
    cc.check_closed_form()


@pytest.mark.parametrize("layout", list(cc.POSTING_LAYOUTS))
@pytest.mark.parametrize("n", cc.POSTINGS)
def test_posting_lists_either_side_of_the_15_bit_count_fields(engine, n, layout):
    """(A launch of these lists outside the groups takes 3.2 s, nearly all of it the set-up's count of a k-mer's pairs with itself:
    countcheck.postings_in_groups.)"""
    cc.run_postings(engine, n, layout)

"""The distance stage where a pair's count meets a border — min_cov against the counting sketch's switches (2, 10, 200), counts against the
ranges of its counters (12, 15, 255) and against the 15-bit count fields of the exact table (32767) — on the host-emulated kernels: the
cases of tests/countcheck.py, every one of which selects edges, against the oracle.  tests/test_gpu_dist_counts.py runs the same cases
on an MI355X, where the sketch's atomics of different waves interleave, and the posting-border launches that the emulator leaves out
(countcheck.postings_in_groups says which and why)."""
import pytest

import countcheck as cc
from centroflye_amd.engine import Engine

BASE = dict(dist_slots=2048, dist_block=128)      # (a small distance kernel: the emulator's time per launch goes with its threads and LDS)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
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
    is taken back.  Seen on the emulator with a line printed where the sweep looks at its wrap word (a scratch build, not kept): with
    4-bit counters (min_cov 2 and 9) every n >= 16 reports the wrap and the first k-mer is swept again with bytes — n = 11 .. 15 do not —
    and n = 256 and 257 then wrap the bytes too and go on to "every b marked", as they do straight away at min_cov 10 and under
    dist_sketch_bits=8; 255 adds do not wrap a byte.  The emulator runs the lanes of a wave one after the other, so a lane's take-backs
    come before the next lane's adds: lane 3 still sees 12 .. 15 and reports the wrap, as the hardware's lanes do together."""
    cc.run_burst(engine, n, min_cov)


def test_the_histogram_written_down_for_the_posting_lists_is_the_oracles(engine):
    cc.check_closed_form()


# (the other launches of this border take ten minutes of set-up each on the emulator: countcheck.postings_in_groups; the MI355X runs them all)
@pytest.mark.parametrize("n, layout", [(n, layout) for n in cc.POSTINGS for layout in cc.POSTING_LAYOUTS if cc.postings_refused(n, layout) or cc.postings_in_groups(n, layout)])
def test_posting_lists_either_side_of_the_15_bit_count_fields(engine, n, layout):
    cc.run_postings(engine, n, layout)

"""Greedy read placement on a real MI355X on hand-built clouds at the capacities of its kernels: the bodies of tests/placecheck.py,
the same that tests/test_emu_place_shapes.py runs on the host emulator, every line against oracle.placer on place_mode 1, 2 and 3.
What only hardware can do — a claim on a score row or on a contig word lost to another lane and taken back — happens here, if it
happens, in the cases that put many lanes on one bucket in one launch (regions that fill up, reads with hundreds of hot rows, several
units of one read laying the same k-mer down); the tests assert results, nothing shows that the branch ran.
Every knob is restored in a `finally` (placecheck.run).  Nothing here reads anything outside the repository."""
import pytest

import placecheck
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


@pytest.mark.parametrize("n", placecheck.POSTING_COUNTS)
def test_posting_rows_and_their_continuation(eng, n):
    placecheck.check_posting_rows(eng, n)


def test_posting_rows_of_64_words_forced_on_short_lists(eng):
    placecheck.check_posting_rows(eng, 31, knobs={"place_row_words": 64})


@pytest.mark.parametrize("n", [32, 65, 200])
def test_posting_rows_of_32_words_forced_on_long_lists(eng, n):
    """(the rows widen by themselves from 32 postings on: the continuation behind a row of 32 words runs only under the knob)"""
    placecheck.check_posting_rows(eng, n, knobs={"place_row_words": 32})


@pytest.mark.parametrize("by", ["seed", "laid"])
@pytest.mark.parametrize("n", placecheck.DIRTY_COUNTS)
def test_dirty_list_of_one_tail(eng, n, by):
    placecheck.check_dirty_list(eng, n, by)


def test_more_touched_blocks_than_the_fused_sweep_holds(eng):
    placecheck.check_touched_blocks(eng)


@pytest.mark.parametrize("n_rows", placecheck.HOT_ROW_COUNTS)
def test_reads_with_many_hot_rows(eng, n_rows):
    placecheck.check_heavy_rows(eng, n_rows)


def test_more_heavy_reads_than_the_heavy_list_holds(eng):
    placecheck.check_many_heavy_reads(eng)


@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("n_pos", [4, 5, 9])
def test_contig_records_and_their_overflow_map(eng, n_pos, f):
    placecheck.check_contig_records(eng, n_pos, f)


@pytest.mark.parametrize("knobs", [None, {"place_slots_per_unit": 1}])
@pytest.mark.parametrize("when", ["seed", "laid"])
def test_score_regions_that_fill_up(eng, when, knobs):
    placecheck.check_score_regions(eng, when, knobs)


@pytest.mark.parametrize("max_units", placecheck.UNIT_COUNTS)
def test_reads_of_one_to_nine_units(eng, max_units):
    placecheck.check_unit_counts(eng, max_units)


@pytest.mark.parametrize("rank", ["shuffled", "reversed"])
def test_ties_across_blocks_go_by_rank(eng, rank):
    placecheck.check_ties(eng, rank)


def test_order_and_thresholds(eng):
    placecheck.check_order_and_thresholds(eng)


def test_stages(eng):
    placecheck.check_stages(eng)


@pytest.mark.parametrize("n", placecheck.BIG_CLOUDS)
def test_clouds_larger_than_their_units(eng, n):
    placecheck.check_big_clouds(eng, n)

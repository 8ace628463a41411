"""Greedy read placement (cf_place2.hip, cf_place.hip as place_mode 1 and as the fall-back) on the host emulator, on hand-built
clouds at the capacities of its kernels: the bodies of tests/placecheck.py, which tests/test_gpu_place_shapes.py runs on an MI355X.
Every line against oracle.placer; every case proves from its own traced restatement that it is where it claims to be."""
import pytest

import placecheck
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_cport_is_the_python_oracle_on_every_small_case():
    """oracle.cport.place_reads (plain C) stands in for oracle.placer where Python is too slow: pinned to it on every small case here."""
    cases = placecheck.small_cases()
    assert len(cases) > 80
    for case in cases:
        assert case.want_cport() == case.want(), case.name


def test_traced_restatement_is_the_python_oracle_on_every_small_case():
    for case in placecheck.small_cases():
        case.traced()


@pytest.mark.parametrize("n", placecheck.POSTING_COUNTS)
def test_posting_rows_and_their_continuation(engine, n):
    placecheck.check_posting_rows(engine, n)


def test_posting_rows_of_64_words_forced_on_short_lists(engine):
    placecheck.check_posting_rows(engine, 31, knobs={"place_row_words": 64})


@pytest.mark.parametrize("n", [32, 65, 200])
def test_posting_rows_of_32_words_forced_on_long_lists(engine, n):
    """(the rows widen by themselves from 32 postings on: the continuation behind a row of 32 words runs only under the knob)"""
    placecheck.check_posting_rows(engine, n, knobs={"place_row_words": 32})


@pytest.mark.parametrize("by", ["seed", "laid"])
@pytest.mark.parametrize("n", placecheck.DIRTY_COUNTS)
def test_dirty_list_of_one_tail(engine, n, by):
    placecheck.check_dirty_list(engine, n, by)


def test_more_touched_blocks_than_the_fused_sweep_holds(engine):
    placecheck.check_touched_blocks(engine, modes=(2,))


@pytest.mark.parametrize("n_rows", placecheck.HOT_ROW_COUNTS)
def test_reads_with_many_hot_rows(engine, n_rows):
    placecheck.check_heavy_rows(engine, n_rows)


def test_more_heavy_reads_than_the_heavy_list_holds(engine):
    placecheck.check_many_heavy_reads(engine)


@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("n_pos", [4, 5, 9])
def test_contig_records_and_their_overflow_map(engine, n_pos, f):
    placecheck.check_contig_records(engine, n_pos, f)


@pytest.mark.parametrize("knobs", [None, {"place_slots_per_unit": 1}])
@pytest.mark.parametrize("when", ["seed", "laid"])
def test_score_regions_that_fill_up(engine, when, knobs):
    placecheck.check_score_regions(engine, when, knobs)


@pytest.mark.parametrize("max_units", placecheck.UNIT_COUNTS)
def test_reads_of_one_to_nine_units(engine, max_units):
    placecheck.check_unit_counts(engine, max_units)


@pytest.mark.parametrize("rank", ["shuffled", "reversed"])
def test_ties_across_blocks_go_by_rank(engine, rank):
    placecheck.check_ties(engine, rank, modes=placecheck.MODES if rank == "shuffled" else (2,))


def test_order_and_thresholds(engine):
    placecheck.check_order_and_thresholds(engine)


def test_stages(engine):
    placecheck.check_stages(engine)


@pytest.mark.parametrize("n", placecheck.BIG_CLOUDS)
def test_clouds_larger_than_their_units(engine, n):
    placecheck.check_big_clouds(engine, n)

"""cf_contig_build / cf_map_reads (cf_map.hip) on the host emulator, on hand-built clouds at the kernels' shape borders: the bodies of
tests/mapshapecheck.py, which tests/test_gpu_map_shapes.py runs on an MI355X.  Every answer against the numpy statements of
tests/mapcheck.py and tests/scorecheck.py; every case proves from numpy alone that it is where it claims to be."""
import pytest

import mapshapecheck as ms
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


# ---- 1. window borders
@pytest.mark.parametrize("span", ms.SPANS)
@pytest.mark.parametrize("window", ms.WINDOWS)
def test_hits_that_span_the_window_and_one_start_more(engine, window, span):
    ms.check_window_border(engine, window, span)


# ---- 2. the admissible range
def test_hits_at_the_last_start_and_one_past_it_and_at_start_zero_and_before_it(engine):
    case, window = ms.last_start_case()
    ms.check(engine, case, window)


@pytest.mark.parametrize("long", [False, True])
def test_best_score_beyond_the_last_start_of_a_contig_with_a_gap(engine, long):
    ms.check(engine, ms.gap_case(long))


def test_thresholds_at_the_score_and_one_above(engine):
    ms.check(engine, ms.threshold_case())


# ---- 3. lane strides and rows
@pytest.mark.parametrize("n_entries", ms.UNIT_ENTRIES)
def test_units_whose_entries_all_hit_one_start(engine, n_entries):
    ms.check(engine, ms.unit_entries_case(n_entries))


@pytest.mark.parametrize("n_positions", ms.ROW_POSITIONS)
def test_rows_of_one_two_and_hundreds_of_positions(engine, n_positions):
    ms.check(engine, ms.row_case(n_positions))


def test_reads_of_one_and_300_units_with_empty_clouds_and_backbone_reads_as_queries(engine):
    ms.check(engine, ms.long_read_case())


# ---- 4. more queries than workgroups
def test_more_queries_than_launched_workgroups(engine):
    fig = ms.check_past_the_launch_cap(engine)
    assert fig["queries"] > 3 * fig["workgroups"]


# ---- 5. the contig builder
@pytest.mark.parametrize("f", ms.RUN_F)
def test_runs_of_f_records_and_one_less_and_one_more(engine, f):
    ms.check_runs(engine, f)


def test_a_rank_frequent_at_one_position_and_present_at_another(engine):
    ms.check(engine, ms.elsewhere_case(), reverse=True)


@pytest.mark.parametrize("f", [16, 10 ** 6])
def test_f_beyond_the_record_count(engine, f):
    ms.check(engine, ms.f_beyond_case(f), reverse=True)


@pytest.mark.parametrize("K,used", [(1, "first"), (50, "first"), (50, "last")])
def test_one_rank_in_use(engine, K, used):
    ms.check(engine, ms.rank_case(K, used), reverse=True)


def test_sort_keys_of_8_to_26_bits(engine):
    assert ms.check_key_widths(engine) == [8, 9, 10, 16, 17, 18, 24, 25, 26]


@pytest.mark.parametrize("n_records", ms.RECORD_COUNTS)
def test_record_counts_around_one_radix_tile(engine, n_records):
    ms.check_record_count(engine, n_records)


def test_more_records_than_threads_and_more_backbone_reads_than_waves(engine):
    fig = ms.check_more_records_than_threads(engine)
    assert fig["records"] == 8 * fig["n_cu"] * 4 * 256 + 77 and fig["backbone_reads"] > 8 * fig["n_cu"] * 4 * 4


def test_coverage_of_300_on_one_position(engine):
    ms.check(engine, ms.coverage_case(), reverse=True)

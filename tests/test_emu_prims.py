"""The bodies of tests/primcheck.py on the host emulator: the record sort, the 32-bit scan, the 64-bit scan in place and the
digit offsets of cf_prims.hip, one call of one primitive each, integer-exact against numpy.  tests/test_gpu_prims.py runs the
same bodies on an MI355X and adds the sizes that only make sense there."""
import pytest

import primcheck
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_tiles_are_the_borders_the_cases_are_built_around(engine):
    primcheck.check_tiles(engine)


# ------------------------------------------------------------------ the record sort
@pytest.mark.parametrize("size", primcheck.SORT_SIZES, ids=primcheck.size_id)
def test_record_sort_sizes(engine, size):
    primcheck.sort_sizes(engine, size)


def test_record_sort_digit_patterns_inside_a_wave(engine):
    primcheck.sort_wave_patterns(engine)


def test_record_sort_is_stable(engine):
    primcheck.sort_stability(engine)


def test_record_sort_odd_and_even_numbers_of_passes(engine):
    primcheck.sort_pass_parity(engine)


@pytest.mark.parametrize("b", primcheck.MONO_BITS)
def test_record_sort_fields_of_the_monokmer_rounds(engine, b):
    primcheck.sort_monokmer_fields(engine, b)


@pytest.mark.parametrize("kbits", [1, 11, 20, 32])
def test_record_sort_fields_of_the_edge_sort(engine, kbits):
    primcheck.sort_edge_fields(engine, kbits)


@pytest.mark.parametrize("nb", [1, 5, 255, 256])
def test_record_sort_fields_of_the_tandem_scan(engine, nb):
    primcheck.sort_tandem_fields(engine, nb)


def test_record_sort_contract_of_bits(engine):
    primcheck.sort_bits_contract(engine)


def test_record_sort_histogram_scan_of_more_than_one_block(engine):
    primcheck.sort_many_tiles(engine, 9)


# ------------------------------------------------------------------ the scans
@pytest.mark.parametrize("size", primcheck.SCAN_SMALL + primcheck.SCAN_SQUARE, ids=primcheck.size_id)
def test_scan_of_32_bit_counts(engine, size):
    primcheck.scan_u32(engine, size)


@pytest.mark.parametrize("size", [(0, 0, 0), (0, 1, 1), (0, 48, 1699)] + primcheck.SCAN_THIRD, ids=primcheck.size_id)
def test_scan_of_64_bit_values_in_place_and_out_of_place(engine, size):
    primcheck.scan_i64_and_inplace(engine, size)


# ------------------------------------------------------------------ the digit offsets
@pytest.mark.parametrize("D", primcheck.DIGITS)
def test_digit_offsets(engine, D):
    primcheck.digit_offsets(engine, D)


def test_digit_offsets_of_all_zero_counts_and_of_one_full_digit(engine):
    primcheck.digit_offsets_special_counts(engine)


def test_digit_offsets_refusals_and_no_tiles(engine):
    primcheck.digit_offsets_refusals(engine)

"""tests/xchcheck.py on the host-emulated build of the kernels: the bucketing, the merge and the mask kernels of the table exchange
for virtual worlds of more than one rank, and the four wrong restatements that the comparison has to notice.  The emulator runs
lanes one after another: it checks the logic of the ballots, shuffles and atomics, not their behaviour in a wave —
tests/test_gpu_exchange.py runs the same bodies on an MI355X."""
import pytest

import xchcheck
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def _dense_sizes(engine):
    return xchcheck.dense_sizes(8 * engine.device_info()["n_cu"])


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("i", range(8))
def test_dense_table_bucketed_for_every_world(engine, i):
    xchcheck.check_table_case(engine, xchcheck.dense_case(_dense_sizes(engine)[i]))


@pytest.mark.parametrize("n_windows", [5, 3000])
def test_hash_table_bucketed_for_every_world(engine, n_windows):
    xchcheck.check_table_case(engine, xchcheck.hash_case(n_windows, 15, n_windows))


def test_poly_a_and_poly_t_reach_their_owners(engine):
    xchcheck.check_table_case(engine, xchcheck.extremes_case())


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("i", range(len(xchcheck.merge_cases())))
def test_records_merge_into_exact_sums(engine, i):
    xchcheck.check_merge(engine, xchcheck.merge_cases()[i])


@pytest.mark.parametrize("parts", [1, 2, 5])
def test_merge_table_leaves_the_same_table(engine, parts):
    for case in xchcheck.merge_cases():
        xchcheck.check_merge(engine, case, parts=parts)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("W", sorted(xchcheck.SHARDS))
def test_whole_exchange_with_virtual_ranks(engine, W):
    xchcheck.check_exchange(engine, W)


# ------------------------------------------------------------------ D
def test_merge_table_refusals(engine, emu_lib):
    with Engine(0, emu_lib) as fresh:
        xchcheck.check_merge_table_refusals(engine, fresh)


@pytest.mark.parametrize("n", xchcheck.MASK_SIZES)
def test_or_unique_mask_against_numpy(engine, n):
    xchcheck.check_or_unique_mask(engine, n)


# ------------------------------------------------------------------ the comparison notices a wrong restatement
def test_owner_shift_of_32_fails(engine):
    xchcheck.check_table_case(engine, xchcheck.dense_case(257), worlds=(3,))
    with pytest.raises(AssertionError, match="W=3: (start|a record lies)"):
        xchcheck.check_table_case(engine, xchcheck.dense_case(257), worlds=(3,), wrong="shift32")


def test_a_run_that_starts_one_record_late_fails(engine):
    with pytest.raises(AssertionError, match="W=3: start"):
        xchcheck.check_table_case(engine, xchcheck.dense_case(257), worlds=(3,), wrong="run_start")


def test_duplicates_that_overwrite_fail(engine):
    with pytest.raises(AssertionError, match="of 300 keys differ"):
        xchcheck.check_merge(engine, xchcheck.copies_case(2, "blocks"), wrong="overwrite")


def test_multi_added_into_the_low_half_fails(engine):
    with pytest.raises(AssertionError, match="of 300 keys differ"):
        xchcheck.check_merge(engine, xchcheck.copies_case(2, "blocks"), wrong="multi_low")

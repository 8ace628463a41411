"""-m gpu: tests/xchcheck.py on a real MI355X — the device code of the table exchange that a world of one rank never reaches, run
for virtual worlds on one engine, with no communicator.  cf_xch_bucket_kernel takes one round per distinct owner of a wave
(ballot, ffs, shuffle, one LDS atomic, rank by popcount under the lane mask) and lays the counts out owner-major;
cf_xch_merge_kernel's lanes race for a slot with atomicCAS and add into a slot another lane claimed; cf_bits_or_kernel sets bits
that the local mask lacks.  The host emulator (test_emu_exchange.py) takes lanes one after another and cannot show a wave-level
mistake in any of them.  Integer-exact throughout; every case asserts its regime from the restatement before the device runs."""
import pytest

import xchcheck
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


# ------------------------------------------------------------------ A
def test_dense_tables_bucketed_for_every_world(engine):
    """1 .. 257 keys (a last wave partly past the table's end, most workgroups past it) for W = 1 .. 257."""
    sizes = xchcheck.dense_sizes(8 * engine.device_info()["n_cu"])
    for n in sizes[:-1]:
        xchcheck.check_table_case(engine, xchcheck.dense_case(n))


def test_dense_table_where_one_workgroup_gets_one_slot(engine):
    """256 g + 1 keys on g workgroups: chunks of 512 slots, workgroup g / 2 scans a single slot, those behind it none."""
    g = 8 * engine.device_info()["n_cu"]
    assert xchcheck.dense_sizes(g)[-1] == 256 * g + 1
    xchcheck.check_table_case(engine, xchcheck.dense_case(256 * g + 1))


@pytest.mark.parametrize("n_windows", [5, 3000])
def test_hash_table_bucketed_for_every_world(engine, n_windows):
    xchcheck.check_table_case(engine, xchcheck.hash_case(n_windows, 15, n_windows))


def test_poly_a_and_poly_t_reach_their_owners(engine):
    xchcheck.check_table_case(engine, xchcheck.extremes_case())


# ------------------------------------------------------------------ B
def test_records_merge_into_exact_sums(engine):
    for case in xchcheck.merge_cases():
        xchcheck.check_merge(engine, case)


@pytest.mark.parametrize("parts", [1, 2, 5])
def test_merge_table_leaves_the_same_table(engine, parts):
    for case in xchcheck.merge_cases():
        xchcheck.check_merge(engine, case, parts=parts)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("W", sorted(xchcheck.SHARDS))
def test_whole_exchange_with_virtual_ranks(engine, W):
    xchcheck.check_exchange(engine, W)


# ------------------------------------------------------------------ D
def test_merge_table_refusals(engine):
    with Engine(0) as fresh:
        xchcheck.check_merge_table_refusals(engine, fresh)


@pytest.mark.parametrize("n", xchcheck.MASK_SIZES)
def test_or_unique_mask_against_numpy(engine, n):
    xchcheck.check_or_unique_mask(engine, n)

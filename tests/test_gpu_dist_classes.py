"""-m gpu: first k-mers with equal posting lists swept once (knob dist_classes) on a real MI355X — the cases of tests/classcheck.py, each
with the knob at 1 and at 0, against the plain restatement, in the launch shapes the library picks by itself (the host emulator of
test_emu_dist_classes.py runs them with two waves per workgroup)."""
import pytest

import classcheck as cc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("min_cov", [1, 2, 4])
def test_classes_of_2_and_3_members_that_select_each_other_and_near_misses(engine, min_cov):
    cc.run(engine, cc.case("core", min_cov=min_cov))


@pytest.mark.parametrize("bits", [1, 3])
def test_different_lists_with_one_hash_are_not_merged(engine, bits):
    """One or three hash bits: the six different lists that begin in unit 0 of read 0 collide; the comparison of the lists decides."""
    cc.run(engine, cc.case("core"), dict(dist_class_bits=bits))
    cc.run(engine, cc.case("big"), dict(dist_class_bits=bits))


def test_a_run_of_equal_lists_longer_than_the_member_cap(engine):
    st = cc.run(engine, cc.case("big"))
    assert st["n_dist_passes"] < len(cc.case("big")["naive"]["kmers"])


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_core_reads_in_the_other_layouts(engine, layout):
    cc.run(engine, cc.case("core"), cc.LAYOUTS[layout])


@pytest.mark.parametrize("block", [128, 0])
def test_a_class_whose_table_splits(engine, block):
    st = cc.run(engine, cc.case("big", min_cov=2), dict(dist_slots=256, dist_block=block))
    assert st["n_spilled"] > 0


@pytest.mark.parametrize("min_cov", [2, 4])
def test_rows_of_a_class_across_edge_chunks_with_marked_slot_sweep_and_in_scan_filter(engine, min_cov):
    cc.run(engine, cc.case("rows", min_cov=min_cov), cc.TIGHT)
    cc.run(engine, cc.case("rows", min_cov=min_cov), dict(dist_edge_chunk=16))


def test_edge_cap_below_the_rows(engine):
    cc.run(engine, cc.case("rows"), edge_cap=50)
    cc.run(engine, cc.case("rows"), cc.TIGHT, edge_cap=50)


def test_two_partitions_split_the_members_of_one_list(engine):
    c = cc.case("core")
    assert [g for g in c["classes"] if len({x % 2 for x in g}) == 2], "a list whose k-mers fall into both partitions"
    cc.run(engine, c, n_parts=2)
    cc.run(engine, cc.case("big"), n_parts=2)


@pytest.mark.parametrize("doubled", [True, False])
def test_a_repeated_rank_in_a_row_switches_the_classes_off(engine, doubled):
    """The results with a class of 2 next to a doubled rank, and of the same clouds as sets (the diagnostic build's test shows which of the
    two launches formed the class)."""
    cc.run_repeated_rank(engine, doubled)


def test_generator_reads_through_the_exchange_path(tmp_path):
    cc.run_exchange(None, str(tmp_path / "rdv"))

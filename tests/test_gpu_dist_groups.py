"""-m gpu: first k-mers of one first posting unit swept together over the union of their lists (knob dist_groups) on a real
MI355X — the cases of tests/groupcheck.py, each with the knob at 1 and at 0, against the plain restatement, in the launch shapes the
library picks by itself (the host emulator of test_emu_dist_groups.py runs them with two waves per workgroup)."""
import pytest

import classcheck as cc
import groupcheck as gc
import sketchtailcheck as stc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("min_cov", [1, 2, 4])
def test_subset_disjoint_and_equal_members_and_pairs_that_only_the_union_or_one_member_reaches(engine, min_cov):
    c = gc.case("core", min_cov=min_cov)
    st = gc.run(engine, c)
    if min_cov >= 2:      # (min_cov 1 runs without the sketch: the launch keeps the classes, the fall-back)
        gc.check_ran_in_groups(c, st)


@pytest.mark.parametrize("params", [dict(min_d=2), dict(max_d=3), dict(min_d=2, max_d=5, min_cov=2)])
def test_min_d_and_a_max_d_below_one_read(engine, params):
    gc.run(engine, gc.case("core", **params))


@pytest.mark.parametrize("name", ["u32", "u33"])
def test_unions_of_32_and_33_postings_and_a_list_of_33_on_its_own(engine, name):
    for c in (gc.case(name), gc.case(name, min_cov=2)):
        gc.check_ran_in_groups(c, gc.run(engine, c))


@pytest.mark.parametrize("cap", [2, 5])
def test_a_small_cap_closes_the_groups_early(engine, cap):
    for c in (gc.case("core"), gc.case("u32")):
        gc.check_ran_in_groups(c, gc.run(engine, c, dict(dist_group_cap=cap)), cap)


@pytest.mark.parametrize("layout", list(gc.LAYOUTS))
def test_core_reads_in_the_other_layouts(engine, layout):
    """wide, region and 26-bit-stream layouts keep the classes (the fall-back); one workgroup per CU runs the groups."""
    gc.run(engine, gc.case("core"), gc.LAYOUTS[layout])


@pytest.mark.parametrize("block", [128, 0])
def test_a_union_table_that_splits(engine, block):
    st = gc.run(engine, cc.case("big", min_cov=2), dict(dist_slots=256, dist_block=block))
    assert st["n_spilled"] > 0
    gc.check_ran_in_groups(cc.case("big", min_cov=2), st)      # (groups whose members differ, from the naive clouds; the passes are not pinned when a table split)


@pytest.mark.parametrize("min_cov", [2, 4])
def test_rows_across_edge_chunks_with_a_hot_list_and_a_stage_that_overflow(engine, min_cov):
    for c in (cc.case("rows", min_cov=min_cov), gc.case("core", min_cov=min_cov)):
        gc.check_ran_in_groups(c, gc.run(engine, c, gc.TIGHT))


def test_edge_cap_below_the_rows(engine):
    c = cc.case("rows")
    gc.check_ran_in_groups(c, gc.run(engine, c, edge_cap=50))
    gc.check_ran_in_groups(c, gc.run(engine, c, gc.TIGHT, edge_cap=50))


def test_tail_items_beyond_d_star_of_the_union(engine):
    """sketchtailcheck's reads: A shares unit 0 of read 0 with other k-mers of other lists — a group whose sketch sweep stops at d*(U), not d*(A)."""
    c = stc.case("core")
    (a,) = stc._ranks(c["naive"], stc.reads_of(stc.core_layout()[0], 500, 21)[2], [stc.A])
    assert [g for g in gc.mixed_groups(c) if a in g[0]], "A in a group with k-mers of other lists"
    gc.check_ran_in_groups(c, gc.run(engine, c))
    gc.check_ran_in_groups(c, gc.run(engine, c, dict(dist_sketch_tail=0)))


def test_two_partitions(engine):
    c = gc.case("core")
    planted = max(c["groups"], key=lambda g: len(g[0]))[0]
    assert len(planted) >= 8 and len({x % 2 for x in planted}) == 2, "the members of the planted group fall into both partitions"
    assert gc.expected_passes(c, part=0, n_parts=2) + gc.expected_passes(c, part=1, n_parts=2) < len({us for us in cc.posting_lists(c["naive"]).values()})
    gc.run(engine, c, n_parts=2)
    gc.run(engine, gc.case("u32"), n_parts=2)


@pytest.mark.parametrize("doubled", [True, False])
def test_a_repeated_rank_in_a_row_makes_every_first_kmer_count_alone(engine, doubled):
    gc.run_repeated_rank(engine, doubled)


def test_generator_reads_through_the_exchange_path(tmp_path):
    gc.run_exchange(None, str(tmp_path / "rdv"))

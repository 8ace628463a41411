"""-m gpu: the sketch sweep cut at d*(a) (knob dist_sketch_tail) on a real MI355X — the cases of tests/sketchtailcheck.py, each with the
knob at 1 and at 0, against the plain restatement, in the launch shapes the library picks by itself (the host emulator of
test_emu_dist_sketch_tail.py runs them with two waves per workgroup)."""
import pytest

import sketchtailcheck as stc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("params", stc.PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_core_reads_under_the_stage_parameters(engine, params):
    stc.run(engine, stc.case("core", **params))


@pytest.mark.parametrize("min_cov", [2, 4])
def test_posting_lists_of_16_17_64_and_65(engine, min_cov):
    stc.run(engine, stc.case("postings", min_cov=min_cov))


@pytest.mark.parametrize("layout", list(stc.LAYOUTS))
def test_core_reads_in_the_other_layouts(engine, layout):
    stc.run(engine, stc.case("core"), stc.LAYOUTS[layout])


@pytest.mark.parametrize("block", [128, 0])
def test_core_reads_with_a_table_that_splits(engine, block):
    st = stc.run(engine, stc.case("core", min_cov=2), dict(dist_slots=256, dist_block=block))
    assert st["n_spilled"] > 0


def test_a_repeated_rank_in_a_row_switches_the_cut_off(engine):
    stc.run_repeated_rank(engine)


def test_generator_reads_through_the_exchange_path(tmp_path):
    stc.run_exchange(None, str(tmp_path / "rdv"))

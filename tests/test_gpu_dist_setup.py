"""-m gpu: the distance set-up with groups (cf_group_walk_kernel, cf_group_fill_kernel) on a real MI355X — the cases of
tests/setupcheck.py against the plain restatement, in the launch shapes the library picks by itself.  (v_readlane, the ballots and the
wave's LDS rows behave on the device in ways the host emulator does not show.)"""
import pytest

import groupcheck as gc
import setupcheck as sc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_setup_case(engine, name):
    sc.CASES[name](engine)


def test_clouds_that_are_not_sets(engine):
    """Every first k-mer a counting group of one: the walk writes the flags and still sums the emissions."""
    gc.run_repeated_rank(engine)

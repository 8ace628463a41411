"""The distance set-up with groups (cf_group_walk_kernel, cf_group_fill_kernel) on the host emulator: the cases of
tests/setupcheck.py against the plain restatement.  Two waves per workgroup (dist_block 128)."""
import pytest

import groupcheck as gc
import setupcheck as sc
from centroflye_amd.engine import Engine

BASE = dict(dist_slots=2048, dist_block=128)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_setup_case(engine, name):
    sc.CASES[name](engine)


def test_clouds_that_are_not_sets(engine):
    """Every first k-mer a counting group of one: the walk writes the flags and still sums the emissions."""
    gc.run_repeated_rank(engine)

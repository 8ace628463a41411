"""The one-section member filter of the distance kernel (knob dist_filter_once) on the host emulator: the cases of
tests/memberfiltercheck.py, each with the knob at 1 and at 0, against the plain restatement.  Two waves per workgroup (dist_block 128)."""
import pytest

import groupcheck as gc
import memberfiltercheck as mf
from centroflye_amd.engine import Engine

BASE = dict(dist_slots=2048, dist_block=128)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(mf.CASES))
def test_member_filter_case(engine, name):
    mf.CASES[name](engine)


def test_counting_groups_of_clouds_that_are_not_sets(engine):
    for once in (1, 0):
        with engine.knobs(dist_filter_once=once):
            gc.run_repeated_rank(engine)

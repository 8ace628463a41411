"""-m gpu: the one-section member filter of the distance kernel (knob dist_filter_once) on a real MI355X — the cases of
tests/memberfiltercheck.py, each with the knob at 1 and at 0, against the plain restatement, in the launch shapes the library picks by
itself.  (v_readlane, the ballots and the barriers of the section behave on the device in ways the host emulator does not show.)"""
import pytest

import groupcheck as gc
import memberfiltercheck as mf
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(mf.CASES))
def test_member_filter_case(engine, name):
    mf.CASES[name](engine)


def test_counting_groups_of_clouds_that_are_not_sets(engine):
    for once in (1, 0):
        with engine.knobs(dist_filter_once=once):
            gc.run_repeated_rank(engine)

"""-m gpu: the group walk with the union in an LDS table and with the union in the lanes (knob dist_walk 1 and 0) on a real
MI355X — the cases of tests/walkcheck.py against the plain restatement, in the launch shapes the library picks by itself.  (The LDS
compare-and-swap of the inserts, the `or` nobody waits for and the lanes' divergent probes behave on the device in ways the host
emulator does not show.)"""
import pytest

import setupcheck as sc
import walkcheck as wc
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)   # raises if libcfhip.so or the GPU is missing: no fallback
    yield e
    e.close()


@pytest.mark.parametrize("knob", wc.KNOB)
@pytest.mark.parametrize("name", sorted(wc.NEW))
def test_walk_case(engine, name, knob):
    wc.run_new(engine, name, knob)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_setup_case_with_the_union_in_the_lanes(engine, name):
    wc.run_setup_knob_0(engine, name)


@pytest.mark.parametrize("knob", wc.KNOB)
def test_clouds_that_are_not_sets(engine, knob):
    wc.run_not_sets(engine, knob)

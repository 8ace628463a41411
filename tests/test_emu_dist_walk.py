"""The group walk with the union in an LDS table and with the union in the lanes (knob dist_walk 1 and 0) on the host
emulator: the cases of tests/walkcheck.py against the plain restatement.  Two waves per workgroup of the distance kernel (dist_block 128)."""
import pytest

import setupcheck as sc
import walkcheck as wc
from centroflye_amd.engine import Engine

BASE = dict(dist_slots=2048, dist_block=128)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
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


def test_the_switch_is_found_by_name_and_not_listed(emu_lib):
    """dist_walk is an A/B switch (cf_knobs.h, CF_KNOB_AB): set and read by name, 1 in a fresh context, stored as 0 or 1, restored by
    Engine.knobs, and absent from the list of tuning knobs that cf_param_name gives."""
    with Engine(0, emu_lib) as e:
        assert e.get_param("dist_walk") == 1 and "dist_walk" not in e.param_names()
        for v, want in ((0, 0), (5, 1), (-3, 1), (0, 0), (1, 1)):
            e.set_param("dist_walk", v)
            assert e.get_param("dist_walk") == want, v
        with e.knobs(dist_walk=0):
            assert e.get_param("dist_walk") == 0
        assert e.get_param("dist_walk") == 1

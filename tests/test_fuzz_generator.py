"""The case generator of tools/fuzz_parity.py (the stage-2 fuzz of the -m gpu suite): every drawn read set varies its error model,
and every knob name and value the generator can set is one the library takes — a refused value would count as "refused", not
as a failure, and the path it was meant to reach would go untested without a word."""
import importlib.util
import os

import numpy as np
import pytest

from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = dict(p_sub=(0.003, 0.04), p_del=(0.003, 0.03), p_ins=(0.003, 0.03), unit_div=(0.003, 0.03))


@pytest.fixture(scope="module")
def fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)      # (the run itself is behind __main__)
    return mod


def test_every_case_draws_its_error_rates(fuzz):
    rng = np.random.default_rng(7)
    seen = {k: set() for k in RANGES}
    for _ in range(300):
        sy, p, part, n_parts, knobs = fuzz.draw_case(rng)
        for k, (lo, hi) in RANGES.items():
            assert k in sy and lo <= sy[k] <= hi, (k, sy)
            seen[k].add(sy[k])
        assert 0 <= part < n_parts
        assert set(knobs) <= set(dict(fuzz.KNOB_CHOICES)), knobs
    assert all(len(v) == 300 for v in seen.values())      # (drawn per case, not fixed)


def test_every_knob_name_and_value_is_accepted(fuzz, emu_lib):
    e = Engine(0, emu_lib)
    try:
        choices = dict(fuzz.KNOB_CHOICES)
        assert set(choices) <= set(e.param_names())
        for name, values in choices.items():
            for v in values:
                e.set_param(name, v)      # (raises DeviceError on a refusal)
    finally:
        e.close()

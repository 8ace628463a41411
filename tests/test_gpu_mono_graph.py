"""The drop-ins of the cen6 pipeline's correction and graph stages (centroflye_amd/mono_error_correction.py, debruijn_graph.py) on a
real MI355X against the reference's records (tests/golden/mono_graph_cases.json): every graph and iterative case, the large read
set included (300 reads of a 12-letter HOR x 60, k = 8 .. 30), which takes minutes on the emulator and is left to this file."""
import pytest

import monographcheck as gc
from test_mono_graph import GOLDEN, MODS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_session():
    from centroflye_amd import session
    from centroflye_amd.engine import Engine
    session.reset()
    session._engine = Engine(0)
    yield session
    session.reset()


def test_the_large_read_set_is_among_the_cases():
    assert sum("strings_seed" in c for c in GOLDEN["graph"]) == 1 and sum("strings_seed" in c for c in GOLDEN["iterative"]) == 1


@pytest.mark.parametrize("case", GOLDEN["graph"], ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_graph_cases_equal_the_reference(gpu_session, case):
    assert gc.run_graph(MODS, case) == case["want"]


@pytest.mark.parametrize("case", GOLDEN["iterative"], ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_iterative_graph_equals_the_reference(gpu_session, case, tmp_path):
    assert gc.run_iterative(MODS, case, str(tmp_path)) == case["want"]


def test_the_gap_correction_cases(gpu_session):
    for case in GOLDEN["correction"]:
        assert gc.run_correction(MODS, case) == case["want"], case["name"]


def test_end_to_end_tsv_to_contigs(gpu_session, tmp_path):
    gc.check_end_to_end(tmp_path, GOLDEN["e2e"])

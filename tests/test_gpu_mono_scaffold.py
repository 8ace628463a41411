"""What follows the graph in the cen6 pipeline (centroflye_amd/debruijn_graph.py: map_reads on cf_monomap.hip, scaffolding,
read2scaffolds, cover_scaffolds_w_reads, extract_read_pseudounits) and the driver's files on a real MI355X against the reference's
records (tests/golden/mono_scaffold_cases.json; tests/test_mono_scaffold.py runs the same on the host emulator)."""
import pytest

import monoscaffoldcheck as sc
from test_mono_scaffold import GOLDEN, MODS, ident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_session():
    from centroflye_amd import session
    from centroflye_amd.engine import Engine
    session.reset()
    session._engine = Engine(0)
    yield session
    session.reset()


@pytest.mark.parametrize("case", GOLDEN["pipeline"], ids=ident)
def test_the_pipeline_behind_the_graph_equals_the_reference(gpu_session, case, tmp_path):
    assert sc.run_pipeline(MODS, case, str(tmp_path)) == case["want"]


def test_the_driver_writes_the_reference_s_results(gpu_session, tmp_path):
    sc.check_end_to_end(tmp_path, GOLDEN["e2e"])

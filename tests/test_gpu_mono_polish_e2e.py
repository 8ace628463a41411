"""The cen6 driver's polishing stage end to end on a real MI355X (scripts/centroFlyeMono.py --stop-after polishing --polisher
consensus): the checks of tests/test_emu_mono_polish_e2e.py with the session's engine on the GPU."""
import pytest

import monopolishcheck as mp

pytestmark = pytest.mark.gpu


@pytest.fixture()
def gpu_session():
    from centroflye_amd import session
    from centroflye_amd.engine import Engine
    session.reset()
    session._engine = Engine(0)
    yield session
    session.reset()


def test_from_the_report_to_the_polished_scaffold(gpu_session, tmp_path):
    from centroflye_amd import centroflye_mono
    figures = mp.check_end_to_end(tmp_path, centroflye_mono.main)
    assert figures["units"] >= 20

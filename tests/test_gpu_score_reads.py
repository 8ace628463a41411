"""cf_score_reads / cf_contig_spread / cf_contig_exact_info (cf_score.hip) on a real MI355X.

  * every golden case of tests/golden/score_reads_cases.json (the REFERENCE's recorded answers: cloud_contig.py's
    calc_inters_score, map_reads and get_spread_kmers) with the default window and with windows of 3 and 1 starts;
  * a seeded hand-built CSR installed through set_clouds, no pipeline run (scorecheck.synthetic_contig): about 5 000 contig
    positions, so a full range takes several windows of the default 2 048; 300 reads of 1 - 120 units whose clouds hold 0 - 150
    ranks; four ranks that recur with a short period.  Full ranges, overhang ranges, sub-ranges, ranges of one start — which must
    give the score the full-range pass gave that start — and cf_contig_spread, all against the numpy statement of
    tests/scorecheck.py, with the default window and with one of 64;
  * one golden case as 192 x n_cu + 5 queries in one call, past the launch cap of 64 x n_cu workgroups, so that every workgroup
    scores several queries in turn on its LDS window.
Nothing here reads the reference tree."""
import pytest

import mapcheck
import scorecheck
from centroflye_amd import session
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu
CASES = scorecheck.load_cases()


@pytest.fixture(scope="module")
def src(report):
    session.reset()
    session._engine = Engine(0)
    yield mapcheck.Sources(session._engine, report, CASES)
    session.reset()


@pytest.mark.parametrize("window", [0, 3, 1])
def test_every_golden_case_on_the_gpu(src, window):
    assert "gfx950" in src.engine.device_info()["name"]
    several = 0
    for case in CASES["cases"]:
        several += scorecheck.check_case(src, case, window=window)
    assert len(CASES["cases"]) >= 50
    assert window == 0 or several > len(CASES["cases"])


@pytest.mark.parametrize("window", [0, 64])
def test_a_hand_built_contig_of_several_windows(window):
    with Engine(0) as e:
        fig = scorecheck.check_synthetic(e, window)
    print(fig)
    assert fig["max_pos"] > 2 * 2048 and fig["mapped"] > 250 and fig["mapped_elsewhere"] >= 1


def test_more_queries_than_launched_workgroups(src):
    """192 x n_cu + 5 queries in one call (49 157 on 256 compute units): every workgroup takes three or four, one after the other
    on the same LDS window."""
    fig = scorecheck.check_past_the_launch_cap(src, next(c for c in CASES["cases"] if c["name"] == scorecheck.STRIDE_CASE))
    print(fig)
    assert fig["queries"] == 192 * fig["n_cu"] + 5 > 3 * fig["workgroups"]

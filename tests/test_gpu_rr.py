"""cf_rr_distances (cf_recruit.hip) on a real MI355X at the limits of its launch shape, the bodies of tests/rrcheck.py: units of
1 .. 4096 bases — 64 blocks, so the last lane of the wave shift carries a block and writes the result — reads at the chunk borders
of the text loop, thresholds at the distance itself and empty reads inside a batch against the REFERENCE's recorded distances
(tests/golden/rr_limits.json); 48 x n_cu + 37 reads in one call, three times what gives every launched wave one item, and exactly
16 x n_cu, against oracle.rr; scripts/rr.py on as many reads.  Nothing here reads the reference tree."""
import os
import subprocess
import sys

import pytest

import rrcheck
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = rrcheck.load_golden()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


def test_block_counts_1_to_64_and_the_refusals_around_them(eng):
    assert rrcheck.check_block_counts(eng, G) == 2 * 2 * 7 * len(rrcheck.BLOCK_UNITS)


def test_chunk_borders_of_the_text_loop(eng):
    assert rrcheck.check_chunk_borders(eng, G) >= 2 * 2 * 20 * len(rrcheck.CHUNK_UNITS)


def test_threshold_at_the_distance_itself(eng):
    assert rrcheck.check_threshold_edge(eng, G) >= 2 * 4 * 5 * len(rrcheck.EDGE_UNITS)


def test_empty_reads_in_the_middle_of_a_batch(eng):
    rrcheck.check_empty_reads_inside_a_batch(eng, G)


def test_more_items_than_launched_waves(eng):
    fig = rrcheck.check_more_items_than_waves(eng)
    print(fig)
    assert fig["reads"] == 48 * fig["n_cu"] + 37 and fig["items"] > 3 * fig["launched_waves"]


def test_the_command_line_on_more_reads_than_waves(eng, tmp_path):
    unit, named, k, want = rrcheck.cli_case(eng.device_info()["n_cu"])
    up, rp = rrcheck.write_cli_input(str(tmp_path), unit, named)
    out = os.path.join(str(tmp_path), "out.fasta")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rr.py"), up, rp, out, str(k)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(out, "rb").read() == want

"""cf_rr_distances (cf_recruit.hip) on the host emulator at the limits of its launch shape, the bodies of tests/rrcheck.py: units
of 1 .. 4096 bases (the 64th lane included) and the refusals around them, reads at the chunk borders of the text loop, thresholds
at the distance itself, empty reads inside a batch — all against the REFERENCE's recorded distances
(tests/golden/rr_limits.json, vendored edlib through tests/golden/make_golden_rr.py) — then more (read, strand) items than the
launch has waves, so that every wave takes several, through the C ABI and through read_recruitment.recruit, against oracle.rr;
and the plain-C restatement itself pinned to the recorded distances up to 64 blocks."""
import os

import pytest

import rrcheck
from centroflye_amd import read_recruitment
from centroflye_amd.engine import Engine
from oracle import rr

G = rrcheck.load_golden()


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_recorded_distances_are_sound_and_small():
    rrcheck.check_golden_is_sound(G)
    assert os.path.getsize(rrcheck.GOLDEN) * 4 < os.path.getsize(os.path.join(os.path.dirname(rrcheck.GOLDEN), "rr_vectors.json"))


def test_oracle_against_the_recorded_distances_up_to_64_blocks():
    assert rrcheck.check_oracle_on_limits(G) >= 1400
    if rr.ref_distance(b"ACGT", b"ACGT", -1) is not None:      # the library itself as well where it was built
        assert rrcheck.reference_limits(rr.ref_distance) == G


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
    assert fig["reads"] == 48 * fig["n_cu"] + 37


def test_recruit_writes_what_the_oracle_selects(eng, tmp_path):
    unit, named, k, want = rrcheck.cli_case(eng.device_info()["n_cu"])
    up, rp = rrcheck.write_cli_input(str(tmp_path), unit, named)
    out = os.path.join(str(tmp_path), "out.fasta")
    seen, kept = read_recruitment.recruit(read_recruitment.read_first_seq(up), rp, out, k, engine=eng)
    assert open(out, "rb").read() == want
    assert (seen, kept) == (len(named), want.count(b">"))

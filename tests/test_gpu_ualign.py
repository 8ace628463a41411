"""The built-in tandem aligner (cf_ualign.hip) on a real MI355X against the rule's plain-Python restatement (tests/ualigncheck.py;
tests/test_emu_ualign.py pins the restatement itself): the literal cases, unit lengths on the borders of a thread's 16 columns, a
wave's 1 024 and the block's 4 096, one base more refused, read lengths 0, 1, m - 1, m, m + 1 and around the row chunk, both strands
winning inside one call, reads of N only, more pairs than a launch has workgroups, batches down to one pair and below one pair's
area, one pair of 2 055 x 6 000 at the generator's error rates between flanks, every refusal, the scratch hygiene, and
scripts/run_ncrf_parallel.py --aligner builtin end to end on the `tiny` and `hor2055` fixtures without an NCRF on PATH, followed by
stage 2 and stage 3."""
import os
import subprocess
import sys

import pytest

import fixtures
import ualigncheck as uc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_literal_cases(eng):
    for case in uc.LITERALS:
        assert uc.check_literal(*case), case[0]
    uc.check_literals(eng)


def test_the_small_seeded_cases(eng):
    for u, r, scores in uc.small_cases()[:60]:
        uc.check(eng, u, [r], scores, uc.align)


@pytest.mark.parametrize("lengths", [uc.UNIT_LENGTHS[:11]] + [(m,) for m in uc.UNIT_LENGTHS[11:]], ids=lambda t: "-".join(map(str, t)) if len(t) < 3 else "1-to-257")
def test_unit_lengths_on_the_borders_of_thread_wave_and_block(eng, lengths):
    assert uc.UNIT_LENGTHS[10] == 257 and len(uc.UNIT_LENGTHS) == 15
    uc.check_unit_lengths(eng, lengths, 40, around_all=True)      # read lengths m - 1, m, m + 1 of every unit length


def test_a_unit_of_4097_bases_is_refused(eng):
    from centroflye_amd.engine import DeviceError
    uc.check_too_long(eng, DeviceError)


def test_read_lengths_around_the_row_chunk(eng):
    uc.check_row_chunks(eng)


def test_more_pairs_than_the_launch_cap(eng):
    assert eng.ualign_info()["launch_cap"] >= 256
    uc.check_more_pairs_than_the_launch_cap(eng)


def test_batches_down_to_one_pair_and_below_one_pairs_area(eng):
    uc.check_batches(eng)


def test_one_pair_of_2055_by_6000_between_flanks(eng):
    uc.check_workload_pair(eng, 2055, 6000)


def test_each_refusal_leaves_the_context_and_the_last_results(eng):
    from centroflye_amd.engine import DeviceError
    uc.check_refusals(eng, DeviceError)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    from centroflye_amd.engine import DeviceError
    uc.check_hygiene(eng, DeviceError)


def _run(script, args, tmp_path):
    empty = tmp_path / "no_ncrf_here"
    empty.mkdir(exist_ok=True)
    return subprocess.run([sys.executable, "-u", os.path.join(SCRIPTS, script)] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PATH=str(empty)))


@pytest.mark.parametrize("fixture", ["tiny", "hor2055"])
def test_the_stage_end_to_end_without_ncrf(report, golden, tmp_path, fixture):
    from centroflye_amd.ncrf_parser import NCRF_Report
    unit, reads, _ = uc.reads_of_fixture(report(fixture), uc.FIXTURE_SEED[fixture])
    uc.write_fasta(tmp_path / "reads.fasta", reads)
    uc.write_fasta(tmp_path / "unit.fasta", [("unit", unit)])
    out = tmp_path / "NCRF"
    r = _run("run_ncrf_parallel.py", ["--reads", tmp_path / "reads.fasta", "--repeat", tmp_path / "unit.fasta", "-t", 3, "-o", out, "--aligner", "builtin"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.listdir(out) == ["report.ncrf"]
    with open(out / "report.ncrf", "rb") as f:
        text = f.read().decode("latin-1")
    wants = uc.check_report(text, unit, reads)      # 1 - 4
    assert sum(w is not None for w in wants) == len(reads)
    rep = NCRF_Report(str(out / "report.ncrf"))      # 5
    assert sorted(rep.records) == sorted(n for n, _ in reads)
    assert all(len(v) >= 2 for v in rep.get_motif_alignments(1).values())
    assert uc.quality(str(out / "report.ncrf"), report(fixture), reads) == (uc.END_SLACK[fixture], uc.UNIT_SLACK[fixture])
    # 6: stage 2 and stage 3 run on it to the end
    p2 = fixtures.stage2_params(fixture)
    out2 = tmp_path / "recruited"
    r = _run("distance_based_kmer_recruitment.py", ["--ncrf", out / "report.ncrf", "--coverage", p2["coverage"], "--min-coverage", p2["min_coverage"], "--outdir", out2,
                                                    "-k", p2["k"], "--max-distance", p2["max_distance"], "--min-distance", p2["min_distance"]], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    kfile = out2 / f"unique_kmers_min_edge_cov_{p2['min_coverage']}.txt"
    p3 = golden(fixture)["stage3"]
    r = _run("read_placer.py", ["--ncrf", out / "report.ncrf", "--genomic-kmers", kfile, "--outdir", tmp_path / "tr", "--n-motif", p3["n_motif"],
                                "--min-cloud-kmer-freq", p3["min_cloud_kmer_freq"], "--min-kmer-mult", p3["min_kmer_mult"], "--min-unit", p3["min_unit"],
                                "--min-inters", p3["min_inters"], "--prefix-threshold", p3["prefix_threshold"]], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "tr" / "read_positions.csv") as f:
        assert len(f.read().splitlines()) == len(reads)


def test_the_default_aligner_without_its_binary_names_it_and_writes_nothing(tmp_path):
    uc.write_fasta(tmp_path / "reads.fasta", [("r", b"ACGTACGT")])
    uc.write_fasta(tmp_path / "unit.fasta", [("unit", b"ACGT")])
    r = _run("run_ncrf_parallel.py", ["--reads", tmp_path / "reads.fasta", "--repeat", tmp_path / "unit.fasta", "-o", tmp_path / "out"], tmp_path)
    assert r.returncode not in (0, None) and "'NCRF'" in r.stderr
    assert not os.path.exists(tmp_path / "out" / "report.ncrf")

"""The built-in tandem aligner (cf_ualign.hip: cf_ualign_run / _ops / _info) on the host emulator.  There is no reference function
behind it, so the rule's plain-Python restatement (tests/ualigncheck.py) is first pinned: literal cases with both rows, interval,
strand and score written out, seven planted misreadings that each change a literal, and an independent check (plain Smith-Waterman
against the unit written out in a row; the score recomputed from the ops).  Then the kernels are compared with it field by field and
op by op at small shapes, and scripts/run_ncrf_parallel.py --aligner builtin end to end on the first reads of the `tiny` and
`hor2055` fixtures (the emulator runs every lane as a fiber: 0.3 ms per row of a 2 055-base unit).  The shapes of hardware size and
every read of the two fixtures are in tests/test_gpu_ualign.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import ualigncheck as uc
from centroflye_amd import session
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


# ---------------------------------------------------------------- pinning the restatement (CPU only)
def test_the_literal_cases_pin_the_restatement():
    assert len(uc.LITERALS) >= 12
    for case in uc.LITERALS:
        assert uc.check_literal(*case), case[0]
        assert uc.check_literal(*case, aligner=uc.align_np), case[0]
    shows = " ".join(uc.LITERAL_SHOWS.values())
    for what in ("diagonal from column m - 1", "horizontal from column 0 to column m - 1", "m = 1", "shorter than the unit", "'-' winner", "'+' / '-' tie",
                 "different rows", "different columns of one row", "inserted run", "deleted run", "an N and a lower-case", "flanks that are left out",
                 "no hit"):
        assert what in shows, what
    # rows, ops and tallies hang together
    for name, u, r, scores, want in uc.LITERALS:
        got = uc.align(u, r, scores)
        if got is not None:
            assert uc.score_of_ops(got["ops"], scores) == got["score"] and len(got["r_al"]) == len(got["m_al"]) == len(got["ops"])
            assert got["r_al"].replace(b"-", b"") == r[got["r_st"]:got["r_en"]] and got["ops"][0] in (uc.MATCH, uc.MISMATCH)


def test_every_misreading_changes_a_literal():
    kills = uc.killers()
    assert set(kills) == set(uc.WRONG_RULES) and all(kills[w] for w in uc.WRONG_RULES), kills


def test_the_score_is_smith_watermans_against_the_unit_in_a_row():
    cases = uc.small_cases()
    assert len(cases) >= 195 and max(len(u) for u, _, _ in cases) == 12 and max(len(r) for _, r, _ in cases) == 60
    seen = set()
    for u, r, scores in cases:
        got, got_np = uc.align(u, r, scores), uc.align_np(u, r, scores)
        assert got == got_np
        k = uc.copies(len(r), len(u), scores)
        assert (got["score"] if got else 0) == max(uc.sw_score(u * k, r, scores), uc.sw_score(uc.rc(u) * k, r, scores))
        if got:
            assert uc.score_of_ops(got["ops"], scores) == got["score"]
            seen |= set(got["ops"])
    assert seen == {uc.MATCH, uc.MISMATCH, uc.INS, uc.DEL}


# ---------------------------------------------------------------- device == restatement
def test_the_literal_cases_on_the_device(eng):
    uc.check_literals(eng)


def test_the_small_seeded_cases_on_the_device(eng):
    for u, r, scores in uc.small_cases()[:60]:
        uc.check(eng, u, [r], scores, uc.align)


def test_unit_lengths_on_the_borders_of_thread_wave_and_block(eng):
    uc.check_unit_lengths(eng, uc.UNIT_LENGTHS, 40)


def test_a_unit_of_4097_bases_is_refused(eng):
    uc.check_too_long(eng, DeviceError)


def test_read_lengths_around_the_row_chunk(eng):
    uc.check_row_chunks(eng)


def test_more_pairs_than_the_launch_cap(eng):
    uc.check_more_pairs_than_the_launch_cap(eng)


def test_batches_down_to_one_pair_and_below_one_pairs_area(eng):
    uc.check_batches(eng)
    with pytest.raises(DeviceError, match="out of range"):
        eng.set_param("ualign_batch_bytes", -1)


def test_a_2055_base_unit_at_the_generators_error_rates(eng):
    uc.check_workload_pair(eng, 2055, 300)


def test_each_refusal_leaves_the_context_and_the_last_results(eng):
    uc.check_refusals(eng, DeviceError)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    uc.check_hygiene(eng, DeviceError)


def test_scores_that_saturate_the_gap_multiples(eng):
    """gap costs whose multiples leave int32 are saturated; the cells stay those of the rule"""
    rng = np.random.default_rng(17)
    u = uc.rand_seq(rng, 70)
    reads = [uc.tandem_read(rng, u, 120, q & 1, 4) for q in range(3)]
    for scores in ((1 << 20, 1 << 30, (1 << 31) - 1), (7, (1 << 31) - 1, 1 << 27), (1000, 1, 1)):
        uc.check(eng, u, reads, scores, uc.align_np)


@pytest.mark.parametrize("order", ["rev", "rand"])
def test_other_lane_orders_give_the_same_results(order):
    """A missing barrier shows as other values when the emulator runs the lanes of a block in another order."""
    code = ("import ualigncheck as uc\nfrom centroflye_amd import _lib\nfrom centroflye_amd.engine import Engine\n"
            f"e = Engine(0, _lib.load({os.path.join(ROOT, 'tests', 'emu', 'libcfhip_emu.so')!r}))\n"
            "uc.check_literals(e)\nuc.check_unit_lengths(e, (17, 65, 1024, 2055), 30)\nuc.check_batches(e)\n")
    env = dict(os.environ, CF_EMU_ORDER=order, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_on_the_ubsan_build():
    from centroflye_amd import _lib
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        uc.check_literals(e)
        uc.check_unit_lengths(e, (1, 16, 17, 1025), 30)
        rng = np.random.default_rng(17)
        u = uc.rand_seq(rng, 70)
        uc.check(e, u, [uc.tandem_read(rng, u, 90, 1, 4)], (1 << 20, 1 << 30, (1 << 31) - 1), uc.align_np)
        uc.check_hygiene(e, DeviceError, batch_bytes=(100, 0))
    finally:
        e.close()


# ---------------------------------------------------------------- the command line
@pytest.fixture()
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    session._engine.set_param("dist_slots", 2048)
    session._engine.set_param("dist_block", 128)
    yield session
    session.reset()


EMU_READS = {"tiny": 6, "hor2055": 2}


@pytest.mark.parametrize("fixture", ["tiny", "hor2055"])
def test_the_stage_end_to_end_without_ncrf(emu_session, report, golden, tmp_path, monkeypatch, fixture):
    from centroflye_amd import distance_based_kmer_recruitment as dbkr, read_placer, unit_aligner
    from centroflye_amd.ncrf_parser import NCRF_Report
    monkeypatch.setenv("PATH", str(tmp_path / "empty"))      # no NCRF anywhere
    unit, reads, _ = uc.reads_of_fixture(report(fixture), uc.FIXTURE_SEED[fixture])
    reads = reads[:EMU_READS[fixture]]      # (the emulator runs a lane as a fiber: every read of the fixture goes through on the GPU)
    uc.write_fasta(tmp_path / "reads.fasta", reads)
    uc.write_fasta(tmp_path / "unit.fasta", [("unit", unit)])
    out = tmp_path / "NCRF"
    assert unit_aligner.main(["--reads", str(tmp_path / "reads.fasta"), "--repeat", str(tmp_path / "unit.fasta"), "-t", "3", "-o", str(out), "--aligner", "builtin"]) == 0
    assert os.listdir(out) == ["report.ncrf"]
    with open(out / "report.ncrf", "rb") as f:
        text = f.read().decode("latin-1")
    wants = uc.check_report(text, unit, reads)      # 1 - 4
    assert sum(w is not None for w in wants) == len(reads)
    rep = NCRF_Report(str(out / "report.ncrf"))      # 5
    assert sorted(rep.records) == sorted(n for n, _ in reads)
    assert all(len(v) >= 2 for v in rep.get_motif_alignments(1).values())
    end, units = uc.quality(str(out / "report.ncrf"), report(fixture), reads)
    assert end <= uc.END_SLACK[fixture] and units[0] <= uc.UNIT_SLACK[fixture][0] and units[1] <= uc.UNIT_SLACK[fixture][1]
    # 6: stage 2 and stage 3 run on it to the end (the emulator takes a reduced --max-distance, as tests/test_dropin.py does)
    p2 = fixtures.stage2_params(fixture)
    out2 = tmp_path / "recruited"
    dbkr.main(["--ncrf", str(out / "report.ncrf"), "--coverage", str(p2["coverage"]), "--min-coverage", str(p2["min_coverage"]), "--outdir", str(out2),
               "-k", str(p2["k"]), "--max-distance", "2", "--min-distance", str(p2["min_distance"])])
    kfile = out2 / f"unique_kmers_min_edge_cov_{p2['min_coverage']}.txt"
    assert kfile.exists()
    p3 = golden(fixture)["stage3"]
    read_placer.main(["--ncrf", str(out / "report.ncrf"), "--genomic-kmers", str(kfile), "--outdir", str(tmp_path / "tr"), "--n-motif", str(p3["n_motif"]),
                      "--min-cloud-kmer-freq", str(p3["min_cloud_kmer_freq"]), "--min-kmer-mult", str(p3["min_kmer_mult"]), "--min-unit", str(p3["min_unit"]),
                      "--min-inters", str(p3["min_inters"]), "--prefix-threshold", str(p3["prefix_threshold"])])
    with open(tmp_path / "tr" / "read_positions.csv") as f:
        assert len(f.read().splitlines()) == len(reads)


def test_min_length_scores_and_fastq_gz(emu_session, tmp_path):
    import gzip
    from centroflye_amd import unit_aligner
    rng = np.random.default_rng(4)
    unit = uc.rand_seq(rng, 33)
    reads = [(f"r{q}", uc.tandem_read(rng, unit, n, q & 1, 7)) for q, n in enumerate((10, 40, 41, 90, 0))] + [("none", b"NNNN")]
    with gzip.open(tmp_path / "reads.fastq.gz", "wb") as f:
        for name, seq in reads:
            f.write(b"@" + name.encode() + b" comment\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    uc.write_fasta(tmp_path / "unit.fasta", [("unit", unit.lower())])
    out = tmp_path / "o"
    assert unit_aligner.main(["--reads", str(tmp_path / "reads.fastq.gz"), "--repeat", str(tmp_path / "unit.fasta"), "-o", str(out), "--aligner", "builtin",
                              "--match", "5", "--mismatch", "4", "--gap", "3", "--min-length", "38"]) == 0
    with open(out / "report.ncrf", "rb") as f:
        text = f.read().decode("latin-1")
    wants = uc.check_report(text, unit, reads, (5, 4, 3), 38)
    kept = [w is not None and w["r_en"] - w["r_st"] >= 38 for w in wants]
    assert 0 < sum(kept) < sum(w is not None for w in wants)
    with pytest.raises(SystemExit) as ei:
        unit_aligner.main(["--reads", str(tmp_path / "reads.fastq.gz"), "--repeat", str(tmp_path / "unit.fasta"), "-o", str(tmp_path / "o2"), "--aligner", "builtin",
                           "--gap", "0"])
    assert "at least 1" in str(ei.value.code) and not os.path.exists(tmp_path / "o2" / "report.ncrf")


def test_the_default_aligner_without_its_binary_names_it_and_writes_nothing(tmp_path, monkeypatch):
    from centroflye_amd import unit_aligner
    monkeypatch.setenv("PATH", str(tmp_path / "empty"))
    uc.write_fasta(tmp_path / "reads.fasta", [("r", b"ACGTACGT")])
    uc.write_fasta(tmp_path / "unit.fasta", [("unit", b"ACGT")])
    for extra, name in (([], "NCRF"), (["--ncrf-bin", "/nonexistent/bin/ncrf_here"], "/nonexistent/bin/ncrf_here")):
        with pytest.raises(SystemExit) as ei:
            unit_aligner.main(["--reads", str(tmp_path / "reads.fasta"), "--repeat", str(tmp_path / "unit.fasta"), "-o", str(tmp_path / "out")] + extra)
        assert ei.value.code not in (0, None) and f"'{name}'" in str(ei.value.code)
        assert not os.path.exists(tmp_path / "out" / "report.ncrf")

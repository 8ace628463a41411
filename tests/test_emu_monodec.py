"""The built-in monomer decomposer (cf_monodec.hip: cf_monodec_run / _get / _info) on the host emulator.  There is no reference
function behind it, so the rule's plain-Python restatement (tests/monodeccheck.py) is first pinned: literal cases with every
instance, op string, score, strand and prefix written out, seven planted misreadings that each change a literal, and an independent
check (the plain global Needleman-Wunsch score of the read against every sequence of monomers; the score recomputed from the ops;
the tiling).  Then the kernels are compared with it, every field and every op count, at small shapes, with monomer borders inside
one thread's 16 columns, on a thread border and one monomer over several threads, both strands in one call; every refusal leaves
the live bytes as they were; and scripts/monomer_decomposer.py runs end to end on a handful of short reads.  The shapes of
hardware size are in tests/test_gpu_monodec.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import monodeccheck as mc
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
    assert len(mc.LITERALS) >= 14
    for case in mc.LITERALS:
        assert mc.check_literal(*case), case[0]
        assert mc.check_literal(*case, decomposer=mc.decompose_np), case[0]
    shows = " ".join(mc.LITERAL_SHOWS.values())
    for what in ("K = 1", "a monomer of length 1", "deleted first bases, through the feedback", "a deleted tail", "an inserted run",
                 "a leading prefix", "going to the smaller k", "'+' / '-' tie going to '+'", "a '-' winner", "an N and a lower-case base",
                 "shorter than every monomer", "n = 0"):
        assert what in shows, what
    ops = "".join(o for c in mc.LITERALS for _, _, _, o in c[4]["inst"])
    assert set(ops) == set("MXID")


def test_every_misreading_changes_a_literal():
    kills = mc.killers()
    assert set(kills) == set(mc.WRONG_RULES) and len(mc.WRONG_RULES) == 7 and all(kills[w] for w in mc.WRONG_RULES), kills


def test_the_score_is_needleman_wunschs_against_the_best_sequence_of_monomers():
    cases = mc.small_cases()
    assert len(cases) >= 200 and max(len(m) for ms, _, _ in cases for m in ms) == 4 and max(len(ms) for ms, _, _ in cases) == 3
    assert max(len(r) for _, r, _ in cases) == 6
    seen, with_prefix = set(), 0
    for monos, r, scores in cases:
        got = mc.decompose(monos, r, scores)
        assert got == mc.decompose_np(monos, r, scores)
        mc.check_invariants(monos, r, scores, got)      # the tiling, the op counts, the ops add up to the score
        assert got["score"] == (mc.brute_score(monos, r, scores) if r else 0)
        seen |= set("".join(o for _, _, _, o in got["inst"]))
        with_prefix += got["prefix"] > 0
    assert seen == set("MXID") and with_prefix >= 10


# ---------------------------------------------------------------- device == restatement
def test_the_literal_cases_on_the_device(eng):
    mc.check_literals(eng)


def test_the_small_seeded_cases_on_the_device(eng):
    for monos, r, scores in mc.small_cases()[:80]:
        mc.check(eng, monos, [r], scores, mc.decompose)


@pytest.mark.parametrize("L,cuts", mc.SMALL_COLUMNS, ids=lambda v: str(v).replace(" ", ""))
def test_columns_on_the_borders_of_a_thread_and_a_wave(eng, L, cuts):
    assert sorted({L for L, _ in mc.SMALL_COLUMNS}) == [1, 2, 15, 16, 17, 63, 64, 65, 257]
    info, wants = mc.check_columns(eng, L, cuts)
    if L >= 15:
        assert {w["strand"] for w in wants[:3]} == {0, 1}      # both strands win inside one call
    assert eng.monodec_info()["n_cols"] == L and eng.monodec_info()["n_monomers"] == len(cuts) + 1


def test_more_columns_than_the_block_holds_are_refused(eng):
    rng = np.random.default_rng(3)
    shape = eng.monodec_info()
    assert (shape["max_cols"], shape["cols_per_thread"], shape["block"], shape["row_chunk"]) == (4096, 16, 256, 1024)
    live = eng.stats()["hbm_bytes_live"]
    with pytest.raises(DeviceError, match="more than 4096 bases"):
        eng.monodec([mc.rand_seq(rng, 4000), mc.rand_seq(rng, 97)], b"ACGT", [0, 4])
    assert eng.stats()["hbm_bytes_live"] == live


def test_read_lengths_0_1_and_around_the_row_chunk(eng):
    mc.check_row_chunks(eng)


def test_more_pairs_than_the_launch_cap(eng):
    mc.check_more_pairs_than_the_launch_cap(eng)


def test_batches_down_to_one_pair_and_below_one_pairs_area(eng):
    mc.check_batches(eng)
    with pytest.raises(DeviceError, match="out of range"):
        eng.set_param("monodec_batch_bytes", -1)


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    mc.check_refusals(eng, DeviceError)


def test_gap_costs_up_to_the_int32_limit(eng):
    mc.check_saturating(eng)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    mc.check_hygiene(eng)


@pytest.mark.parametrize("order", ["rev", "rand"])
def test_other_lane_orders_give_the_same_results(order):
    """A missing barrier shows as other values when the emulator runs the lanes of a block in another order."""
    code = ("import monodeccheck as mc\nfrom centroflye_amd import _lib\nfrom centroflye_amd.engine import Engine\n"
            f"e = Engine(0, _lib.load({os.path.join(ROOT, 'tests', 'emu', 'libcfhip_emu.so')!r}))\n"
            "mc.check_literals(e)\n[mc.check_columns(e, L, cuts) for L, cuts in mc.SMALL_COLUMNS[5:]]\nmc.check_columns(e, 1100, [300, 1024, 1030])\nmc.check_batches(e)\n")
    env = dict(os.environ, CF_EMU_ORDER=order, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_on_the_ubsan_build():
    from centroflye_amd import _lib
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        mc.check_literals(e)
        for L, cuts in mc.SMALL_COLUMNS[6:]:
            mc.check_columns(e, L, cuts)
        mc.check_saturating(e)
        e.set_param("monodec_batch_bytes", 100)
        mc.check_hygiene(e)
    finally:
        e.close()


# ---------------------------------------------------------------- the command line
@pytest.fixture()
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


def short_reads():
    rng = np.random.default_rng(77)
    monomers = [(b"mono_%d" % k, mc.rand_seq(rng, n)) for k, n in enumerate((31, 40, 29, 36))]
    seqs = [s for _, s in monomers]
    reads = [(b"short_%d" % q, mc.noisy_read(rng, seqs, 5, q & 1, err=0.08, start=q % 4)) for q in range(5)]
    reads.append((b"tiny_one", b"ACGTNNacgt"))
    return monomers, reads


def test_the_command_line_end_to_end(emu_session, tmp_path):
    from centroflye_amd import monomer_decomposer
    monomers, reads = short_reads()
    results = [mc.decompose_np([s for _, s in monomers], r) for _, r in reads]
    rep = mc.check_cli_and_parser(tmp_path, monomers, reads, results, monomer_decomposer.main)
    assert set(rep.monostrings) <= {n.decode() for n, _ in reads} and len(rep.monostrings) >= 5
    assert {ms.strand for ms in rep.monostrings.values()} == {"+", "-"}
    for (name, r), res in zip(reads[:5], results[:5]):
        ms = rep.monostrings[name.decode()]
        assert len(ms.string) >= 4 and set(ms.tostring()) <= set("ABCD?")
        for coord, (c, a, b) in ms.mono2nucl.items():
            assert 0 <= min(a, b) <= max(a, b) < len(r)


def test_other_scores_min_identity_and_fastq_gz(emu_session, tmp_path):
    import gzip
    from centroflye_amd import monomer_decomposer
    monomers, reads = short_reads()
    with gzip.open(tmp_path / "reads.fastq.gz", "wb") as f:
        for name, r in reads:
            f.write(b"@" + name + b" x\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    mc.write_fasta(tmp_path / "monomers.fasta", monomers)
    out = tmp_path / "out.tsv"
    assert monomer_decomposer.main(["--sequences", str(tmp_path / "reads.fastq.gz"), "--monomers", str(tmp_path / "monomers.fasta"), "-o", str(out),
                                    "--match", "2", "--mismatch", "3", "--gap", "4", "--min-identity", "93"]) == 0
    results = [mc.decompose_np([s for _, s in monomers], r, (2, 3, 4)) for _, r in reads]
    with open(out) as f:
        text = f.read()
    assert text == mc.tsv_lines([n.decode() for n, _ in reads], [n.decode() for n, _ in monomers], results, None, 93)
    assert "\t?\n" in text and "\t+\n" in text


def test_a_refusal_exits_non_zero_and_writes_no_file(emu_session, tmp_path):
    from centroflye_amd import monomer_decomposer
    monomers, reads = short_reads()
    mc.write_fasta(tmp_path / "reads.fasta", reads)
    mc.write_fasta(tmp_path / "monomers.fasta", monomers)
    mc.write_fasta(tmp_path / "bad.fasta", monomers + [(b"odd", b"ACGTNACGT")])
    for args in (["-m", str(tmp_path / "monomers.fasta"), "--gap", "0"], ["-m", str(tmp_path / "bad.fasta")],
                 ["-m", str(tmp_path / "monomers.fasta"), "--match", str(1 << 30)]):
        with pytest.raises(SystemExit) as e:
            monomer_decomposer.main(["-s", str(tmp_path / "reads.fasta"), "-o", str(tmp_path / "d.tsv")] + args)
        assert e.value.code not in (0, None)
        assert sorted(os.listdir(tmp_path)) == ["bad.fasta", "monomers.fasta", "reads.fasta"]

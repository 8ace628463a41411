"""The built-in monomer decomposer (cf_monodec.hip) on a real MI355X against the rule's plain-Python restatement
(tests/monodeccheck.py; tests/test_emu_monodec.py pins the restatement itself): the literal cases, column counts on the borders of
a thread's 16 columns, a wave's 1 024 and the block's 4 096 (the borders asserted from cf_monodec_info), one column more refused, a
monomer border on the wave border, one monomer of 2 000 bases, K = L and K = 1, read lengths 0, 1 and around the row chunk, more
pairs than a launch has workgroups, batches down to one pair and below one pair's area, gap costs at the int32 limit, the scratch
hygiene, one read of 6 000 bases at the generator's error rates against the 18 D6Z1 monomers, and the end-to-end check
decomposer -> decomposition.tsv -> SD_Report on D6Z1-shaped reads with a planted monomer deletion."""
import numpy as np
import pytest

import monodeccheck as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_literal_cases(eng):
    for case in mc.LITERALS:
        assert mc.check_literal(*case), case[0]
    mc.check_literals(eng)


def test_the_small_seeded_cases(eng):
    for monos, r, scores in mc.small_cases()[:80]:
        mc.check(eng, monos, [r], scores, mc.decompose)


def test_the_small_column_counts(eng):
    for L, cuts in mc.SMALL_COLUMNS:
        mc.check_columns(eng, L, cuts)


# (L, cuts): 255 / 256 / 257 around the first launch of more than 64 threads' columns x 4; 1 024 / 1 025 around a wave's columns;
# 4 095 / 4 096 at the block's; monomer borders on the wave border 1 024 and next to it; one monomer of 2 000 bases; K = L; K = 1
BIG_COLUMNS = [(255, [100, 240]), (256, [16, 17, 255]), (257, [256]), (1024, [500, 1000]), (1025, [1024]), (2100, [1024, 1030, 2048]),
               (2300, [100, 2100]), (4095, [170, 1023, 1024, 1025, 3000]), (4096, [2048, 4095]), (4096, []), (1030, list(range(1, 1030)))]


@pytest.mark.parametrize("L,cuts", BIG_COLUMNS, ids=lambda v: str(v) if isinstance(v, int) else ("cuts%d" % len(v)))
def test_columns_on_the_borders_of_wave_and_block(eng, L, cuts):
    shape = eng.monodec_info()
    wave_cols = 64 * shape["cols_per_thread"]
    assert (shape["max_cols"], shape["cols_per_thread"], shape["block"], wave_cols) == (4096, 16, 256, 1024)
    Ls = sorted({L for L, _ in BIG_COLUMNS})
    assert {wave_cols, wave_cols + 1, shape["max_cols"] - 1, shape["max_cols"], 255, 256, 257} <= set(Ls)
    assert 2000 in mc.split_lengths(2300, [100, 2100]) and wave_cols in BIG_COLUMNS[5][1]
    info, wants = mc.check_columns(eng, L, cuts, read_bases=330)
    assert eng.monodec_info()["n_cols"] == L and eng.monodec_info()["n_monomers"] == len(cuts) + 1


def test_the_d6z1_monomers_and_one_read_of_6000_bases(eng):
    seqs = [s for _, s in mc.d6z1_monomers()]
    assert len(seqs) == 18 and sum(len(s) for s in seqs) == 3065
    rng = np.random.default_rng(6000)
    ks = [(5 + x) % 18 for x in range(36)]
    r, _ = mc.hor_read(rng, seqs, ks, 1, mc.RATES)
    r = r[40:6040]
    assert len(r) == 6000
    info, ptr, inst, wants = mc.check(eng, seqs, [r])
    assert wants[0]["strand"] == 1 and 34 <= len(wants[0]["inst"]) <= 37
    ms = eng.monodec_info()["phase_ms"]
    assert ms["score"] > 0.0 and ms["moves"] > 0.0 and ms["total"] >= ms["score"] + ms["moves"]


def test_4097_columns_are_refused(eng):
    from centroflye_amd.engine import DeviceError
    rng = np.random.default_rng(3)
    live = eng.stats()["hbm_bytes_live"]
    for monos in ([mc.rand_seq(rng, 4097)], [mc.rand_seq(rng, 4096), b"A"], [b"A"] * 4097):
        with pytest.raises(DeviceError, match="more than 4096"):
            eng.monodec(monos, b"ACGT", [0, 4])
    assert eng.stats()["hbm_bytes_live"] == live


def test_read_lengths_0_1_and_around_the_row_chunk(eng):
    assert eng.monodec_info()["row_chunk"] == 1024
    mc.check_row_chunks(eng)


def test_more_pairs_than_the_launch_cap(eng):
    assert eng.monodec_info()["launch_cap"] >= 256
    mc.check_more_pairs_than_the_launch_cap(eng)


def test_batches_down_to_one_pair_and_below_one_pairs_area(eng):
    mc.check_batches(eng)


def test_gap_costs_up_to_the_int32_limit(eng):
    mc.check_saturating(eng)


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    from centroflye_amd.engine import DeviceError
    mc.check_refusals(eng, DeviceError)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    mc.check_hygiene(eng)


# the quality of the decomposition of the noisy reads below, computed with the restatement on the CPU and recorded in DESIGN §27:
# (instances, instances whose monomer is the planted one, instances marked '?')
NOISY_QUALITY = (20, 20, 0)


def test_end_to_end_decomposer_tsv_monostrings(eng, tmp_path):
    """reads of five D6Z1 monomers in HOR order with one monomer of the row left out, every other read turned round: four without
    errors, four at the generator's error rates"""
    from centroflye_amd import monomer_decomposer, session
    monomers = mc.d6z1_monomers()
    seqs = [s for _, s in monomers]
    clean, noisy = mc.hor_reads(4, 5, 271), mc.hor_reads(4, 5, 272, mc.RATES)
    reads = clean + noisy
    results = [mc.decompose_np(seqs, r) for _, r, *_ in reads]
    # the restatement alone, on the CPU: every error-free read gives its planted string (none of the 4 is left out)
    for (name, r, ks, strand, _), res in zip(clean, results):
        assert res["strand"] == strand and res["prefix"] == 0 and res["score"] == len(r)
        assert [k for k, *_ in res["inst"]] == (ks[::-1] if strand else ks) and all(set(o) == {"M"} for *_, o in res["inst"])
    assert mc.quality(noisy, results[4:]) == NOISY_QUALITY
    session.reset()
    session._engine = eng
    try:
        rep = mc.check_cli_and_parser(tmp_path, monomers, reads, results, monomer_decomposer.main)      # the TSV, byte for byte
    finally:
        session._engine = None
        session.reset()
    assert list(rep.monostrings) == sorted(n.decode() for n, *_ in reads)
    for name, r, ks, strand, _ in clean:
        ms = rep.monostrings[name.decode()]
        assert ms.tostring() == mc.planted_string(ks) and ms.strand == "-+"[1 - strand]
    for name, r, ks, strand, _ in noisy:
        ms = rep.monostrings[name.decode()]
        assert ms.tostring() == mc.planted_string(ks) and ms.strand == "-+"[1 - strand]      # (all 20 instances right, none marked '?')

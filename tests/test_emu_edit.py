"""cf_edit_distances / cf_hpc / cf_edit_info (cf_edit.hip) on the host emulator against the REFERENCE's recorded answers
(tests/golden/edit_cases.json, captured by tests/golden/make_golden_edit.py from the reference's vendored edlib in mode NW and its
compress_homopolymer): the cases with d^2 <= 10^6 — every length pair around the 8-byte and 64-byte borders, every pair of
start offsets mod 8, 100 000 identical bytes with a mismatch on either side of every border of the cooperative extension, a whole
HOR unit deleted and inserted, pairs on both sides of the LDS/HBM switch of the wavefronts (forced down by the knob), the limit
k, batches — the numpy and Python statements of tests/editcheck.py pinned to the same answers, every refusal followed by a
working call, and the UBSan build."""
import os
import subprocess

import numpy as np
import pytest

import editcheck as ec
from centroflye_amd import _lib
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = ec.load_cases()


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small(eng):
    info = eng.edit_info()
    assert {k: info[k] for k in G["shape"]} == G["shape"], "the goldens straddle other borders than the kernel's: regenerate them"
    return ec.single_cases(info["lane_bytes"], info["turn_bytes"], small_only=True)


def test_the_goldens_tell_every_misreading_from_the_reference():
    assert set(G["wrong_rule_kills"]) == set(ec.WRONG_RULES) and all(v >= 1 for v in G["wrong_rule_kills"].values())
    a, b = b"ACGTNNACGTacgtNACGT", b"ACGTACACGTACGTNNCGT"
    want = G["single"]["N_and_case"]["distance"]
    assert ec.nw(a, b) == want and ec.nw(a, b, "n_matches_anything") < want and ec.nw(a, b, "case_folding") < want
    data, off, seqs = ec.hpc_case(True)
    assert ec.sha(b"".join(ec.hpc(s) for s in seqs)) == G["hpc_long"]["sha_out"]
    assert ec.sha(b"".join(ec.hpc(s, "hpc_resets_at_tile_borders") for s in seqs)) != G["hpc_long"]["sha_out"]
    # the clamp at n: never the distance, always the rows a run reaches
    a, b = b"ACGTACGT", b"ACGTACGTACGTACGT"
    assert ec.fr(a, b, want_reach=True) == (8, 8)
    d, reach = ec.fr(a, b, wrong="no_clamp_at_n", want_reach=True)
    assert d == 8 and reach > 8


def test_the_statements_agree_with_the_reference_on_the_small_cases(small):
    n = 0
    for name, a, b in small:
        if len(a) * len(b) <= 5 * 10 ** 6:
            want = G["single"][name]["distance"]
            assert ec.nw(a, b) == want, name
            if len(a) * len(b) <= 10 ** 5:
                assert ec.fr(a, b) == want and ec.fr(a, b, want - 1) == (-1 if want else 0), name
            n += 1
    assert n >= 70


def test_every_small_case_alone_and_as_one_batch(eng, small):
    assert len(small) >= 64 + 2 + 20 + 4
    ec.check_singles(eng, G, small)


def test_every_pair_of_start_offsets_mod_8(eng):
    cases = ec.offset_cases()
    assert {(c[2][0] % 8, c[3][0] % 8) for c in cases} == {(i, j) for i in range(8) for j in range(8)}
    for name, data, a_off, b_off, a, b in cases:
        assert ec.sha(data) == G["offsets"][name]["sha"]
        d, _ = eng.edit_distances(data, a_off, b_off)
        assert int(d[0]) == G["offsets"][name]["distance"], name


def test_the_limit(eng, small):
    ec.check_limits(eng, G, [c for c in small if c[0] in ("len_65_65", "len_0_9", "len_64_0", "empty_empty", "ident", "ident_mismatch_0",
                                                            "hor171_unit_deleted", "related_1200", "N_and_case")])


@pytest.mark.parametrize("lds_diags", [64, 3, 1])
def test_both_sides_of_the_lds_hbm_switch(eng, small, lds_diags):
    """The knob moves the switch point down so that the pairs around it stay small; the default one is taken on hardware."""
    with eng.knobs(edit_lds_diags=lds_diags):
        assert eng.edit_info()["lds_diags"] == lds_diags
        cases = ec.switch_cases(max(lds_diags, 8))
        for name, a, b in cases:
            assert ec.one_pair(eng, a, b) == ec.nw(a, b), name
        # a batch whose pairs fall on both sides, in one launch
        mixed = [c for c in small if c[0] in ("len_7_9", "len_65_63", "unrelated_600", "hor171_unit_inserted", "related_1200", "len_1_0")] + cases
        aa, bb = b"".join(c[1] for c in mixed), b"".join(c[2] for c in mixed)
        a_off = np.cumsum([0] + [len(c[1]) for c in mixed])
        b_off = np.cumsum([0] + [len(c[2]) for c in mixed]) + len(aa)
        d, _ = eng.edit_distances(aa + bb, a_off, b_off)
        assert d.tolist() == [ec.nw(c[1], c[2]) for c in mixed]
        d, _ = eng.edit_distances(aa + bb, a_off, b_off, 100)
        assert d.tolist() == [w if w <= 100 else -1 for w in (ec.nw(c[1], c[2]) for c in mixed)]
    assert eng.edit_info()["lds_diags"] == G["shape"]["lds_diags"]


def test_batches_of_none_one_and_three_thousand(eng):
    d, ms = eng.edit_distances(b"", [0], [0])
    assert d.size == 0 and ms == 0.0
    d, _ = eng.edit_distances(None, [0], [0])
    assert d.size == 0
    data, a_off, b_off = ec.batch_case()
    assert ec.sha(data) == G["batch"]["sha"] and a_off.size == 3001
    sizes = np.diff(a_off)
    assert sizes.min() >= 150 and sizes.max() <= 2100 and (np.diff(sizes) < 0).sum() > 1000      # shuffled size order
    d, _ = eng.edit_distances(data, a_off[:2], b_off[:2])
    assert d.tolist() == G["batch"]["distances"][:1]
    d, _ = eng.edit_distances(data, a_off, b_off)
    assert d.tolist() == G["batch"]["distances"]
    for p in range(0, 3000, 211):
        assert ec.nw(data[a_off[p]:a_off[p + 1]], data[b_off[p]:b_off[p + 1]]) == G["batch"]["distances"][p]
    d, _ = eng.edit_distances(data, a_off, b_off, 3)
    assert d.tolist() == [w if w <= 3 else -1 for w in G["batch"]["distances"]]


def test_hpc_and_the_resident_bytes(eng):
    for key, long_runs in (("hpc_short", False), ("hpc_long", True)):
        data, off, seqs = ec.hpc_case(long_runs)
        assert ec.sha(data) == G[key]["sha_in"]
        out, out_off = eng.hpc(data, off)
        assert ec.sha(out) == G[key]["sha_out"] and np.diff(out_off).tolist() == G[key]["lengths"]
        assert [out[out_off[i]:out_off[i + 1]].tobytes() for i in range(len(seqs))] == [ec.hpc(s) for s in seqs]
        assert eng.edit_info()["resident_bytes"] == len(data) + out.size
    # the bytes cf_hpc left: every sequence against its successor, plain and compressed, in one call
    every = np.concatenate([off, off[-1] + out_off[1:]])
    strings = seqs + [ec.hpc(s) for s in seqs]
    d, _ = eng.edit_distances(None, every[:-1], every[1:], 50)
    want = []
    for x, y in zip(strings[:-1], strings[1:]):
        w = ec.nw(x, y) if len(x) * len(y) <= 10 ** 6 else (abs(len(x) - len(y)) if abs(len(x) - len(y)) > 50 else None)
        want.append(w if w is None or w <= 50 else -1)
    assert all(w is None or int(g) == w for g, w in zip(d, want)) and sum(w is not None for w in want) >= len(want) - 2
    with pytest.raises(DeviceError, match="beyond the"):
        eng.edit_distances(None, [0, every[-1] + 1], [0, 1])
    # no sequences, empty sequences only
    out, out_off = eng.hpc(b"", [0])
    assert out.size == 0 and out_off.tolist() == [0]
    out, out_off = eng.hpc(b"", [0, 0, 0])
    assert out.size == 0 and out_off.tolist() == [0, 0, 0]
    assert eng.edit_info()["resident_bytes"] == 0
    with pytest.raises(DeviceError, match="none resident"):
        eng.edit_distances(None, [0, 0], [0, 0])


def test_each_refusal_leaves_the_context_usable(emu_lib):
    e = Engine(0, emu_lib)
    try:
        def good():
            return ec.one_pair(e, b"ACGTACGT", b"ACTTACG")
        assert good() == 2
        for args, what in [((b"ACGT", [0, 2], [2, 4], -1), "negative distance limit"),
                           ((b"ACGT", [2, 0], [2, 4]), "decrease"),
                           ((b"ACGT", [-1, 2], [2, 4]), "negative offset")]:
            with pytest.raises(DeviceError, match=what) as ei:
                e.edit_distances(*args)
            assert "(-22)" in str(ei.value)
            assert good() == 2
        with pytest.raises(ValueError, match="beyond the bytes"):
            e.edit_distances(b"ACGT", [0, 2], [2, 5])
        with pytest.raises(ValueError, match="one more"):
            e.edit_distances(b"ACGT", [0, 2], [2])
        off, out_off = np.array([1, 2], np.int64), np.zeros(2, np.int64)
        rc = emu_lib.cf_hpc(e._ctx, None, off.ctypes.data, 1, None, out_off.ctypes.data)
        assert rc == -22 and b"off[0]" in emu_lib.cf_last_error(e._ctx)
        with pytest.raises(DeviceError, match="decrease"):
            e.hpc(b"ACGT", [0, 3, 2, 4])
        with pytest.raises(DeviceError, match="out of range"):
            e.set_param("edit_lds_diags", 16385)
        assert good() == 2
        assert e.times() == {k: 0.0 for k in e.times()} and e.stats()["n_reads"] == 0      # nothing is added to cf_times or cf_stats
    finally:
        e.close()


def test_on_the_ubsan_build(small):
    script = os.path.join(ROOT, "tests", "emu", "build_emu.sh")
    subprocess.check_call(["bash", script], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        e.set_param("edit_lds_diags", 16)
        ec.check_singles(e, G, [c for c in small if c[0].startswith("len_") or c[0] in ("ident_mismatch_4097", "hor171_unit_deleted")])
        data, off, seqs = ec.hpc_case(False)
        out, out_off = e.hpc(data, off)
        assert ec.sha(out) == G["hpc_short"]["sha_out"]
    finally:
        e.close()

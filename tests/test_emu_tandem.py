"""cf_tandem_scan / cf_tandem_hook_positions / cf_tandem_info (cf_tandem.hip) on the host emulator against the REFERENCE's recorded
answers (tests/golden/tandem_cases.json, captured by tests/golden/make_golden_tandem.py from the reference's own unit_extractor
functions): every case of tests/tandemcheck.py — no reads; reads shorter than k, of k and of k + 1 bases; no repeat, one repeat, a
perfect tandem, homopolymers; bin size 0; ties, even and odd best windows, periods[0] != period(best_l); the same k-mer at the end
of one read and the start of the next; runs and distance segments across the tile borders cf_tandem_info reports; k = 1, 15, 16,
31; both key modes; batch borders inside the list; reads with N and lower case; 64 HOR-like reads of 20 kb — the numpy statement
and the mirror module pinned to the same answers, every refusal followed by a working call, and the UBSan build."""
import os
import subprocess

import numpy as np
import pytest

import tandemcheck as tc
from centroflye_amd import _lib
from centroflye_amd import unit_extractor as ue
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = tc.load_cases()
CASES = {c["name"]: c for c in tc.cases()}
SMALL = [n for n in CASES if n != "hor64"]


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_goldens_tell_every_misreading_from_the_reference():
    assert set(G["wrong_rule_kills"]) == set(tc.WRONG_RULES) and all(v >= 1 for v in G["wrong_rule_kills"].values())
    assert set(G["cases"]) == set(CASES)
    f = G["facts"]
    assert f["even_best"] and f["odd_best"] and f["period_differs_from_best_l"] and f["hor_period_off"] <= 10


@pytest.mark.parametrize("name", SMALL)
def test_the_numpy_statement_and_the_mirror_module_agree_with_the_reference(name):
    case, g = CASES[name], G["cases"][name]
    for i, (seq, res, rec) in enumerate(zip(case["reads"], tc.restate_case(case), g["reads"])):
        assert not tc.differs(rec, tc.summary(seq, res, case["k"])), (name, i)
        s = seq.decode("latin-1")
        rep = ue.get_repetitive_kmers(s, case["k"])
        conv, union = ue.get_convolution(rep)
        assert (len(rep), len(union)) == (rec["n_rep_kmers"], rec["n_conv"])
        periods, bin_convs, bl, br = ue.get_period_info(union, case["bin_size"])
        if rec["period"] is None:
            assert (periods, bin_convs, bl, br) == ([], [], None, None)
            continue
        assert (periods[0], bin_convs[0], bl, br) == (rec["period"], rec["count"], rec["bin_left"], rec["bin_right"])
        assert list(periods[:8]) == rec["periods_head"] and list(bin_convs[:8]) == rec["bin_convs_head"] and len(periods) == rec["n_periods"]
        assert tc.sha(__import__("json").dumps([list(periods), list(bin_convs)]).encode()) == rec["tuples_sha"]
        hook = ue.get_hook_kmer(conv, bl, br)
        splits = ue.split_by_hook(s, hook)
        assert hook == rec["hook"] and tc.sha("\n".join(splits).encode()) == rec["split_ids_sha"]
        assert ue.select_template(splits) == (rec["med_len"], rec["template"])


@pytest.mark.parametrize("name", SMALL)
def test_every_small_case_on_the_device(eng, name):
    tc.check_case(eng, G, CASES[name])


def test_the_tiles_case_straddles_every_border_the_kernel_reports(eng):
    info = eng.tandem_info()
    assert {k: info[k] for k in G["shape"]} == G["shape"], "the goldens straddle other borders than the kernel's: regenerate them"
    case = CASES["tiles"]
    wins = np.cumsum([0] + [max(len(s) - case["k"] + 1, 0) for s in case["reads"]])
    dists = np.cumsum([0] + [r["n_conv"] for r in G["cases"]["tiles"]["reads"]])
    homo = [i for i, s in enumerate(case["reads"]) if len(set(s)) == 1]
    for tile in set(G["shape"].values()) | {64}:
        # one run (a homopolymer's windows) and one read's distances with a multiple of the tile strictly inside
        assert any(wins[i] // tile < (wins[i + 1] - 1) // tile for i in homo), tile
        assert any(dists[i] // tile < (dists[i + 1] - 1) // tile for i in range(len(case["reads"]))), tile
    assert wins[-1] > 2 * info["sort_tile"]


@pytest.mark.parametrize("mode", [1, 2])
def test_both_key_modes(eng, mode):
    with eng.knobs(tandem_key_mode=mode):
        for name in SMALL:
            if mode == 1 and CASES[name]["k"] == 31 and CASES[name]["reads"]:
                with pytest.raises(DeviceError, match="more than 64 key bits") as ei:      # 62 code bits leave no byte for a position
                    tc.check_case(eng, G, CASES[name])
                assert "(-22)" in str(ei.value)
                continue
            tc.check_case(eng, G, CASES[name], expect_mode=mode)
    tc.check_case(eng, G, CASES["k_31"], expect_mode=2)      # auto: records where the keys do not fit
    tc.check_case(eng, G, CASES["k_16"], expect_mode=1)


@pytest.mark.parametrize("batch", [1, 37, 1000, 2996, 5992])
def test_batch_borders_inside_the_list(eng, batch):
    with eng.knobs(tandem_batch_windows=batch):
        assert eng.tandem_info()["batch_windows"] == batch
        for name in ("tiles", "noisy_k6_bin3", "read_border", "lengths_around_k", "exotic"):
            tc.check_case(eng, G, CASES[name])
            case = CASES[name]
            wins = [max(len(s) - case["k"] + 1, 0) for s in case["reads"]]
            if sum(wins) > batch:
                assert eng.tandem_info()["n_batches"] > 1
    assert eng.tandem_info()["batch_windows"] == 1 << 26


def test_the_hor_like_reads(eng):
    rows = tc.check_case(eng, G, CASES["hor64"], expect_mode=1)
    assert rows.size == 64 and np.all(np.abs(rows["period"] - 2055) <= 10)
    info = eng.tandem_info()
    assert info["n_batches"] == 1 and info["n_records"] == 64 * (20000 - 14)


def test_each_refusal_leaves_the_context_usable(emu_lib):
    e = Engine(0, emu_lib)
    try:
        case = CASES["perfect_tandem"]
        data, off = tc.pack(case["reads"])

        def good():
            tc.check_case(e, G, case)
            return e.tandem_hook_positions()
        with pytest.raises(DeviceError, match="no cf_tandem_scan before"):
            e.tandem_hook_positions()
        ptr, pos = good()
        for args, what in [((data, off, 0, 10), "k must lie"), ((data, off, 32, 10), "k must lie"), ((data, off, 15, -1), "negative bin"),
                           ((data, [0, 30, 20], 15, 10), "decrease"), ((data, [-1, 20], 15, 10), "negative offset")]:
            with pytest.raises(DeviceError, match=what) as ei:
                e.tandem_scan(*args)
            assert "(-22)" in str(ei.value)
            p2, q2 = e.tandem_hook_positions()      # the results of the call before are still there
            assert np.array_equal(p2, ptr) and np.array_equal(q2, pos)
        rc = emu_lib.cf_tandem_scan(e._ctx, None, off.ctypes.data, -1, 15, 10, None)
        assert rc == -22 and b"negative number of reads" in emu_lib.cf_last_error(e._ctx)
        long_off = np.array([0, 1 << 31], np.int64)      # refused by its length alone: no byte is looked at
        out = np.zeros(1, Engine.TANDEM_DTYPE)
        rc = emu_lib.cf_tandem_scan(e._ctx, data, long_off.ctypes.data, 1, 15, 10, out.ctypes.data)
        assert rc == -22 and b"2^31 bases" in emu_lib.cf_last_error(e._ctx)
        with pytest.raises(ValueError, match="beyond the bytes"):
            e.tandem_scan(b"ACGT", [0, 5], 2, 1)
        for name, value in (("tandem_key_mode", 3), ("tandem_batch_windows", -1)):
            with pytest.raises(DeviceError, match="out of range"):
                e.set_param(name, value)
        good()
        assert e.times() == {k: 0.0 for k in e.times()} and e.stats()["n_reads"] == 0      # nothing is added to cf_times or cf_stats
    finally:
        e.close()


def test_scan_reads_redoes_the_exotic_reads_on_the_host(eng):
    case, g = CASES["exotic"], G["cases"]["exotic"]
    res = ue.scan_reads(case["ids"], [s.decode("latin-1") for s in case["reads"]], case["k"], case["bin_size"], engine=eng)
    assert [r.on_host for r in res] == [tc.is_exotic(s, case["k"]) for s in case["reads"]] and sum(r.on_host for r in res) == 4
    for r, seq, rec in zip(res, case["reads"], g["reads"]):
        if rec["period"] is None:
            assert r.status == "no_period"
            continue
        assert (r.period, r.count, r.bin_left, r.bin_right, r.hook, r.hook_index) == tuple(rec[f] for f in ("period", "count", "bin_left", "bin_right", "hook", "hook_index"))
        splits = ue.splits_from_positions(seq.decode("latin-1"), r.hook_pos)
        assert tc.sha("\n".join(splits).encode()) == rec["split_ids_sha"]


def test_on_the_ubsan_build():
    script = os.path.join(ROOT, "tests", "emu", "build_emu.sh")
    subprocess.check_call(["bash", script], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        for mode in (0, 2):
            e.set_param("tandem_key_mode", mode)
            for name in ("lengths_around_k", "homopolymer", "k_1", "k_16", "k_31", "read_border", "exotic", "no_reads"):
                tc.check_case(e, G, CASES[name])
    finally:
        e.close()

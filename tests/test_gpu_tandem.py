"""cf_tandem_scan / cf_tandem_hook_positions on a real MI355X against the REFERENCE's recorded answers
(tests/golden/tandem_cases.json): every case of the emulator suite — the shapes at the kernels' own tile borders, k = 1, 15, 16, 31,
both key modes, batch borders inside the list, the reads the host has to redo, and the 64 HOR-like reads of 20 kb."""
import numpy as np
import pytest

import tandemcheck as tc
from centroflye_amd import unit_extractor as ue

pytestmark = pytest.mark.gpu
G = tc.load_cases()
CASES = {c["name"]: c for c in tc.cases()}
SMALL = [n for n in CASES if n != "hor64"]


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_goldens_straddle_the_borders_of_this_build(eng):
    info = eng.tandem_info()
    assert {k: info[k] for k in G["shape"]} == G["shape"], "the goldens straddle other borders than the kernel's: regenerate them"
    assert info["batch_windows"] == 1 << 26


@pytest.mark.parametrize("name", SMALL)
def test_every_small_case(eng, name):
    tc.check_case(eng, G, CASES[name])


@pytest.mark.parametrize("mode", [1, 2])
def test_both_key_modes(eng, mode):
    from centroflye_amd.engine import DeviceError
    with eng.knobs(tandem_key_mode=mode):
        for name in SMALL + ["hor64"]:
            if mode == 1 and CASES[name]["k"] == 31 and CASES[name]["reads"]:
                with pytest.raises(DeviceError, match="more than 64 key bits"):
                    tc.check_case(eng, G, CASES[name])
                continue
            tc.check_case(eng, G, CASES[name], expect_mode=mode)
    tc.check_case(eng, G, CASES["k_31"], expect_mode=2)


@pytest.mark.parametrize("batch", [1, 37, 1000, 2996, 5992])
def test_batch_borders_inside_the_list(eng, batch):
    with eng.knobs(tandem_batch_windows=batch):
        for name in ("tiles", "noisy_k6_bin3", "read_border", "lengths_around_k", "exotic"):
            tc.check_case(eng, G, CASES[name])


def test_the_hor_like_reads_in_one_batch_and_in_seven(eng):
    rows = tc.check_case(eng, G, CASES["hor64"], expect_mode=1)
    assert np.all(np.abs(rows["period"] - 2055) <= 10)
    info = eng.tandem_info()
    assert info["n_batches"] == 1 and info["n_records"] == 64 * (20000 - 14) and info["phase_ms"]["total"] > 0.0
    with eng.knobs(tandem_batch_windows=200000):
        again = tc.check_case(eng, G, CASES["hor64"])
        assert eng.tandem_info()["n_batches"] == 7 and np.array_equal(again, rows)


def test_a_refusal_leaves_the_results_of_the_call_before(eng):
    from centroflye_amd.engine import DeviceError
    case = CASES["perfect_tandem"]
    tc.check_case(eng, G, case)
    ptr, pos = eng.tandem_hook_positions()
    data, off = tc.pack(case["reads"])
    with pytest.raises(DeviceError, match="k must lie"):
        eng.tandem_scan(data, off, 32, 10)
    p2, q2 = eng.tandem_hook_positions()
    assert np.array_equal(p2, ptr) and np.array_equal(q2, pos)
    tc.check_case(eng, G, case)


def test_extract_units_writes_the_reference_s_files(eng, tmp_path):
    """The exotic case end to end: the batch on the GPU, the reads with N and lower case on the host, the files by their hashes."""
    case, g = CASES["exotic"], G["cases"]["exotic"]
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">" + i.encode() + b" tail\n" + s + b"\n" for i, s in zip(case["ids"], case["reads"])))
    rows = ue.extract_units(str(fa), str(tmp_path / "out"), case["k"], case["bin_size"], engine=eng)
    assert [r["status"] for r in rows] == ["ok" if rec["period"] is not None else "no_period" for rec in g["reads"]]
    for i, rec in zip(case["ids"], g["reads"]):
        d = tmp_path / "out" / i[:8]
        if rec["period"] is None:
            assert not d.exists()
            continue
        assert tc.sha((d / "splits.fasta").read_bytes()) == rec["splits_sha"]
        assert tc.sha((d / "median_read_unit.fasta").read_bytes()) == rec["median_sha"]

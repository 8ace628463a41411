"""cf_contig_build / cf_map_reads (cf_map.hip) on the host emulator against the REFERENCE's recorded answers
(tests/golden/map_reads_cases.json, captured by tests/golden/make_golden_map_reads.py from cloud_contig.py's own CloudContig and
map_reads_fast): every golden case through the C ABI with the default window and with windows so small that a read takes several,
the numpy statement of tests/mapcheck.py pinned to the same answers, the degenerate inputs, every refusal followed by a working
call, and one fixture on the UBSan build of the emulator."""
import os
import subprocess

import numpy as np
import pytest

import mapcheck
from centroflye_amd import _lib, session
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mapcheck.load_cases()
SOURCES = list(CASES["sources"])


def _session(lib, report):
    session.reset()
    session._engine = Engine(0, lib)
    return mapcheck.Sources(session._engine, report, CASES)


@pytest.fixture(scope="module")
def src(emu_lib, report):
    s = _session(emu_lib, report)
    yield s
    session.reset()


def _cases(source):
    return [c for c in CASES["cases"] if c["source"] == source]


def test_the_goldens_tell_every_wrong_rule_from_the_reference():
    assert set(CASES["wrong_rule_kills"]) == set(mapcheck.WRONG_RULES)
    for rule, per_source in CASES["wrong_rule_kills"].items():
        assert sum(per_source.values()) >= 1, rule
    assert len([c for c in CASES["cases"] if c["name"].startswith("hand_gap")]) == 2
    assert len(CASES["cases"]) >= 3 * 42 + 2 + 2 + 2


@pytest.mark.parametrize("source", SOURCES)
def test_every_golden_case_through_the_c_abi(src, source):
    cases = _cases(source)
    assert cases
    for case in cases:
        mapcheck.check_case(src, case)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("window", [1, 3, 7])
def test_every_golden_case_with_small_windows(src, source, window):
    """A window of 1, 3 or 7 candidate starts: the hits of a read of these fixtures spread over up to ~90 starts (HOR k-mers are
    not unique to one place), so the score table is filled and reduced in several passes."""
    several = 0
    for case in _cases(source):
        several += mapcheck.check_case(src, case, window=window)["multi_window_reads"]
    assert several >= len(_cases(source)), "the cases of this source do not make reads take several windows"


def test_queries_as_a_subset_in_shuffled_order_and_twice(src):
    case = next(c for c in CASES["cases"] if c["name"] == "hor2055_full_t2_10")
    ids, unit_ptr, cloud_ptr, entries = src.use(case["source"])
    e = src.engine
    row = {r: i for i, r in enumerate(ids)}
    e.contig_build([row[r] for r, _ in case["backbone"]], [p for _, p in case["backbone"]], case["f"])
    want = {row[r]: (tuple(v) if v is not None else (-1, 0, 0)) for r, v in case["expect"]["reads"].items()}
    full = e.map_reads(None, case["threshold"])
    assert [tuple(int(a[i]) for a in full) for i in range(len(ids))] == [want[i] for i in range(len(ids))]
    rng = np.random.default_rng(5)
    q = rng.permutation(len(ids))[: len(ids) // 2]
    q = np.concatenate([q, q[:3]])      # (a read may be asked for more than once)
    for _ in range(2):
        got = e.map_reads(q, case["threshold"])
        assert [tuple(int(a[i]) for a in got) for i in range(q.size)] == [want[int(r)] for r in q]
    assert all(a.size == 0 for a in e.map_reads(np.zeros(0, np.int64), case["threshold"]))
    info = e.contig_info()
    e.contig_build([row[r] for r, _ in case["backbone"]][::-1], [p for _, p in case["backbone"]][::-1], case["f"])      # the order plays no part
    again = e.contig_info()
    assert {k: v for k, v in again.items() if not k.endswith("_ms")} == {k: v for k, v in info.items() if not k.endswith("_ms")}
    assert all(np.array_equal(a, b) for a, b in zip(e.map_reads(None, case["threshold"]), full))


def test_empty_backbone_and_a_read_without_units(src):
    ids, unit_ptr, cloud_ptr, entries = src.use("hand")
    e = src.engine
    assert unit_ptr[13] == unit_ptr[12]      # read 12 has no units
    e.contig_build([], [], 2)
    info = e.contig_info()
    assert (info["n_positions"], info["max_pos"], info["n_freq_kmers"], info["n_pairs"]) == (0, 0, 0, 0)
    assert e.contig_coverage().size == 0
    pos, s0, s1 = e.map_reads(None, (1, 1))
    assert (pos == -1).all() and not s0.any() and not s1.any()
    e.contig_build([0, 1, 12], [0, 0, 7], 2)      # a backbone read without units adds nothing, not even a covered position
    assert e.contig_info()["n_positions"] == 8 and e.contig_info()["max_pos"] == 7
    pos, s0, s1 = e.map_reads([12, 0], (1, 1))
    assert pos.tolist() == [-1, 0] and s0.tolist() == [0, 8] and s1.tolist() == [0, 16]
    # thresholds below one do not admit a start without a hit (the reference looks at scored starts only)
    pos, _, _ = e.map_reads([13], (0, 0))
    assert pos.tolist() == [-1]


def test_each_refusal_leaves_the_context_and_the_contig_usable(emu_lib):
    e = Engine(0, emu_lib)
    try:
        spec = CASES["sources"]["hand"]
        a = mapcheck.synthetic_arrays(spec)
        e.load_arrays(a["bases"], a["read_off"], a["unit_ptr"], a["unit_start"], a["unit_end"])
        with pytest.raises(DeviceError, match="no clouds installed"):
            e.contig_build([0], [0], 2)
        with pytest.raises(DeviceError, match="no clouds installed"):
            e.map_reads(None)
        mapcheck.install_synthetic(e, spec)
        with pytest.raises(DeviceError, match="no contig"):
            e.map_reads(None)
        with pytest.raises(DeviceError, match="no contig"):
            e.contig_info()
        R = a["unit_ptr"].size - 1

        def good():
            e.contig_build([0, 1, 4, 5], [0, 0, 8, 8], 2)
            assert e.contig_info()["n_positions"] == 16
            return e.map_reads([9], (2, 2))[0].tolist()
        assert good() == [10]
        for reads, pos, what in [([0, 0], [0, 3], "twice"), ([0, R], [0, 0], "out of range"), ([-1], [0], "out of range"),
                                 ([0, 1], [0, -1], "negative"), ([0], [2 ** 31 - 8], "2\\^31"), ([0], [2 ** 40], "2\\^31")]:
            with pytest.raises(DeviceError, match=what) as ei:
                e.contig_build(reads, pos, 2)
            assert "(-22)" in str(ei.value)
            # the contig of the last good call is still there, and a new one can be built
            assert e.contig_info()["n_positions"] == 16 and e.map_reads([9], (2, 2))[0].tolist() == [10]
            assert good() == [10]
        for q in ([R], [-1]):
            with pytest.raises(DeviceError, match="out of range"):
                e.map_reads(q)
            assert good() == [10]
        with pytest.raises(DeviceError, match="map_window"):
            e.set_param("map_window", 4097)
        # clouds built, filtered or installed again, or reads loaded again, drop the contig
        e.filter_clouds(1)
        with pytest.raises(DeviceError, match="no contig"):
            e.map_reads(None)
        assert good() == [10]
        e.set_clouds(a["cloud_ptr"], a["entries"])
        with pytest.raises(DeviceError, match="no contig"):
            e.contig_coverage()
        assert good() == [10]
        e.load_arrays(a["bases"], a["read_off"], a["unit_ptr"], a["unit_start"], a["unit_end"])
        with pytest.raises(DeviceError, match="no clouds installed"):
            e.map_reads(None)
        mapcheck.install_synthetic(e, spec)
        assert good() == [10]
    finally:
        e.close()


def test_one_fixture_on_the_ubsan_build(report):
    script = os.path.join(ROOT, "tests", "emu", "build_emu.sh")
    subprocess.check_call(["bash", script], env=dict(os.environ, CF_EMU_UBSAN="1"))
    lib = _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so"))
    s = _session(lib, report)
    try:
        for case in _cases("lowcov")[:6] + _cases("hand"):
            mapcheck.check_case(s, case)
            mapcheck.check_case(s, case, window=5)
    finally:
        session.reset()

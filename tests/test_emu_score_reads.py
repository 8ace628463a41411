"""cf_score_reads / cf_contig_spread / cf_contig_exact_info (cf_score.hip) on the host emulator against the REFERENCE's recorded
answers (tests/golden/score_reads_cases.json, captured by tests/golden/make_golden_score_reads.py from cloud_contig.py's own
CloudContig.calc_inters_score, map_reads and get_spread_kmers): every golden case through the C ABI with the default window and
with windows so small that a range takes several, the numpy statement of tests/scorecheck.py pinned to the same answers, queries
as a shuffled subset, more queries than the launch has workgroups, the degenerate reads, every refusal followed by a working call, cf_map_reads unchanged by a score call,
and one fixture on the UBSan build of the emulator."""
import os
import subprocess

import numpy as np
import pytest

import mapcheck
import scorecheck
from centroflye_amd import _lib, session
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = scorecheck.load_cases()
SOURCES = list(dict.fromkeys(c["source"] for c in CASES["cases"]))


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


def _case(name):
    return next(c for c in CASES["cases"] if c["name"] == name)


def test_the_goldens_tell_every_wrong_rule_from_the_reference():
    assert set(CASES["wrong_rule_kills"]) == set(scorecheck.WRONG_RULES) and len(scorecheck.WRONG_RULES) == 7
    for rule, per_source in CASES["wrong_rule_kills"].items():
        assert sum(per_source.values()) >= 1, rule
    assert os.path.getsize(scorecheck.GOLDEN) <= os.path.getsize(scorecheck.MAP_GOLDEN)
    assert [0, 0] in [c["threshold"] for c in CASES["cases"]]
    # the two scorers differ on the hand-built backbones: some read's fast answer is not its exact one
    differ = 0
    for c in _cases("hand"):
        if c["fast"] is not None:
            differ += any((f if f is not None else [-1, 0, 0]) != row[0:3] for f, row in zip(c["fast"].values(), c["reads"]))
    assert differ >= 4


def test_the_keep_rule_on_the_threshold_itself():
    """hand_tie: under (8, 16) the reads 2-7 score exactly (8, 16) at a start other than 0 and are dropped, read 11 scores (5, 10)
    at start 0 and is kept because its start is 0; under (5, 10) the reads 8 and 9 score exactly (5, 10) elsewhere."""
    c = _case("hand_tie_t8_16")
    rows = dict(zip(c["read_ids"], c["reads"]))
    for r in "234567":
        assert rows[r][15:] == [0] and rows[r][1:3] == [8, 16] and rows[r][0] > 0
    assert rows["11"][15:] == [1, 0, 5, 10]
    c = _case("hand_tie_t5_10")
    rows = dict(zip(c["read_ids"], c["reads"]))
    for r in "89":
        assert rows[r][15:] == [0] and rows[r][1:3] == [5, 10] and rows[r][0] > 0


@pytest.mark.parametrize("source", SOURCES)
def test_every_golden_case_through_the_c_abi(src, source):
    cases = _cases(source)
    assert cases
    for case in cases:
        scorecheck.check_case(src, case)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("window", [1, 3, 7])
def test_every_golden_case_with_small_windows(src, source, window):
    several = 0
    for case in _cases(source):
        several += scorecheck.check_case(src, case, window=window)
    assert several >= len(_cases(source)), "the cases of this source do not make ranges take several windows"


def test_queries_as_a_shuffled_subset_with_repeats_and_map_reads_unchanged(src):
    case = _case("hor2055_full_t2_10")
    ids, unit_ptr, cloud_ptr, entries = src.use(case["source"])
    e = src.engine
    row = {r: i for i, r in enumerate(ids)}
    e.contig_build([row[r] for r, _ in case["backbone"]], [p for _, p in case["backbone"]], case["f"])
    fast_before = e.map_reads(None, case["threshold"])
    info_before = e.contig_info()
    want = {row[r]: tuple(w[0:3]) for r, w in zip(case["read_ids"], case["reads"])}
    full = e.score_reads(None, None, None, *case["threshold"])
    assert [tuple(int(a[i]) for a in full) for i in range(len(ids))] == [want[i] for i in range(len(ids))]
    rng = np.random.default_rng(5)
    q = rng.permutation(len(ids))[: len(ids) // 2]
    q = np.concatenate([q, q[:3]])      # (a read may be asked for more than once)
    for _ in range(2):
        got = e.score_reads(q, None, None, *case["threshold"])
        assert [tuple(int(a[i]) for a in got) for i in range(q.size)] == [want[int(r)] for r in q]
    assert all(a.size == 0 for a in e.score_reads(np.zeros(0, np.int64)))
    assert e.contig_exact_info()["score_ms"] >= 0.0
    # the fast mapper's answers and the contig's figures are what they were
    assert all(np.array_equal(a, b) for a, b in zip(e.map_reads(None, case["threshold"]), fast_before))
    after = e.contig_info()
    assert {k: v for k, v in after.items() if not k.endswith("_ms")} == {k: v for k, v in info_before.items() if not k.endswith("_ms")}
    # and the recorded fast answers are the ones compared with
    fast = [tuple(v) if v is not None else (-1, 0, 0) for v in case["fast"].values()]
    assert [tuple(int(a[row[r]]) for a in fast_before) for r in case["read_ids"]] == fast


def test_more_queries_than_launched_workgroups(src):
    """Every workgroup takes three or four queries, one after the other on the same LDS window."""
    fig = scorecheck.check_past_the_launch_cap(src, _case(scorecheck.STRIDE_CASE))
    print(fig)
    assert fig["queries"] == 192 * fig["n_cu"] + 5 > 256


def test_reads_without_units_and_with_empty_clouds(src):
    ids, unit_ptr, cloud_ptr, entries = src.use("hand")
    e = src.engine
    assert unit_ptr[13] == unit_ptr[12] and unit_ptr[14] - unit_ptr[13] == 3 and cloud_ptr[unit_ptr[14]] == cloud_ptr[unit_ptr[13]]
    e.contig_build([0, 1], [0, 0], 2)      # max_pos = 7
    c = scorecheck.contig(unit_ptr, cloud_ptr, entries, [0, 1], [0, 0], 2)
    for t, want in [((0, 0), [(8, 0, 0), (5, 0, 0)]), ((1, 1), [(-1, 0, 0), (-1, 0, 0)])]:
        got = e.score_reads([12, 13], None, None, *t)
        assert [tuple(int(a[i]) for a in got) for i in range(2)] == want
        assert [scorecheck.score_read(unit_ptr, cloud_ptr, entries, c, r, 0, None, *t) for r in (12, 13)] == want
    # a range of its own: the rightmost start, also beyond max_pos; an empty range is None whatever the thresholds are
    got = e.score_reads([12, 13, 0, 0], [2, 3, 9, 4], [40, 3, 30, 3], 0, 0)
    assert got[0].tolist() == [40, 3, 30, -1] and not got[1].any() and not got[2].any()
    got = e.score_reads([12, 13], None, None, -1, -5)
    assert got[0].tolist() == [8, 5]
    # an empty contig: max_pos = 0, no pair
    e.contig_build([], [], 2)
    assert e.contig_exact_info()["n_exact_pairs"] == 0 and e.contig_spread(0).size == 0
    got = e.score_reads(None, None, None, 0, 0)
    n_units = np.diff(unit_ptr)
    assert got[0].tolist() == [int(v) if v >= 0 else -1 for v in (0 - n_units + 1)] and not got[1].any()
    assert (e.score_reads(None, None, None, 1, 1)[0] == -1).all()


def test_each_refusal_leaves_the_context_and_the_contig_usable(emu_lib):
    e = Engine(0, emu_lib)
    try:
        spec = CASES["sources"]["hand"]
        a = mapcheck.synthetic_arrays(spec)
        e.load_arrays(a["bases"], a["read_off"], a["unit_ptr"], a["unit_start"], a["unit_end"])
        with pytest.raises(DeviceError, match="no clouds installed"):
            e.score_reads(None)
        mapcheck.install_synthetic(e, spec)
        for call in (lambda: e.score_reads(None), lambda: e.contig_spread(5), e.contig_exact_info):
            with pytest.raises(DeviceError, match="no contig") as ei:
                call()
            assert "(-22)" in str(ei.value)
        R = a["unit_ptr"].size - 1

        def good():
            e.contig_build([0, 1, 4, 5], [0, 0, 8, 8], 2)
            assert e.contig_exact_info()["n_exact_pairs"] == 32
            return [int(v[0]) for v in e.score_reads([9], None, None, 2, 2)]
        assert good() == [10, 5, 10]
        for q, lo, what in [([R], None, "out of range"), ([-1], None, "out of range"), ([0, 1], [0, -1], "negative first start")]:
            with pytest.raises(DeviceError, match=what) as ei:
                e.score_reads(q, lo, None)
            assert "(-22)" in str(ei.value)
            assert [int(v[0]) for v in e.score_reads([9], None, None, 2, 2)] == [10, 5, 10]      # the contig is still there
            assert good() == [10, 5, 10]
        with pytest.raises(ValueError, match="per query"):
            e.score_reads([0, 1], [0], None)
        # whatever drops the contig drops the exact CSR with it
        e.filter_clouds(1)
        with pytest.raises(DeviceError, match="no contig"):
            e.score_reads(None)
        assert good() == [10, 5, 10]
        e.set_clouds(a["cloud_ptr"], a["entries"])
        with pytest.raises(DeviceError, match="no contig"):
            e.contig_spread(0)
        assert good() == [10, 5, 10]
    finally:
        e.close()


def test_one_fixture_on_the_ubsan_build(report):
    script = os.path.join(ROOT, "tests", "emu", "build_emu.sh")
    subprocess.check_call(["bash", script], env=dict(os.environ, CF_EMU_UBSAN="1"))
    lib = _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so"))
    s = _session(lib, report)
    try:
        for case in _cases("lowcov")[:4] + _cases("hand"):
            scorecheck.check_case(s, case)
            scorecheck.check_case(s, case, window=5)
    finally:
        session.reset()

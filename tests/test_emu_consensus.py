"""The built-in consensus polisher (cf_consensus.hip: cf_consensus_run / _get / _info) on the host emulator.  There is no reference
function behind it, so the rule's plain-Python restatement (tests/conscheck.py) is first pinned by hand-written cases with the
expected bytes written out, and shown to be told apart from five plausible misreadings by those cases; then the kernels are
compared with it byte for byte: the literal cases, template lengths around the wave and the block borders, 1 .. 130 reads per
position, more positions than a launch has workgroups, batches that cut through one position's reads, every refusal followed by
a working call, and scripts/eltr_polisher.py --polisher consensus end to end on the `tiny` fixture.  The shapes of hardware size
(2 055 bases x 32 reads, the longest string taken) are in tests/test_gpu_consensus.py."""
import os
import runpy
import sys

import numpy as np
import pytest

import conscheck as cc
from centroflye_amd import session
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "eltr_polisher.py")


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_literal_cases_pin_the_restatement():
    for name, t, reads, permille, want in cc.LITERALS:
        got = cc.consensus(t, reads, len(want), permille)
        assert [g[0] for g in got] == list(want), name
        if name in cc.LITERAL_COUNTS:
            assert got[0][1:] == cc.LITERAL_COUNTS[name], name
    # the cases the rule's description names, bytes written out once more
    assert cc.consensus(b"ACGT", [b"AGGT", b"ACGT"], 1, 1000)[0][0] == b"ACGT"
    assert cc.consensus(b"ATGT", [b"ACGT", b"AGGT"], 1, 1000)[0][0] == b"ACGT"
    assert cc.consensus(b"ACT", [b"ACGT", b"ACT"], 1, 1000)[0][0] == b"ACT"
    assert cc.consensus(b"ACT", [b"ACGT", b"ACGT", b"ACT"], 1, 1000)[0][0] == b"ACGT"
    # the walk itself: (a) before (b) before (c)
    D = cc.matrix(b"AAT", b"AT")
    assert D.tolist() == [[0, 1, 2], [1, 0, 1], [2, 1, 1], [3, 2, 1]]
    assert cc.walk(D, b"AAT", b"AT") == ([None, ord("A"), ord("T")], {})
    assert cc.walk(cc.matrix(b"AATT", b"AACGCGCTT"), b"AATT", b"AACGCGCTT") == ([65, 65, 84, 84], {2: b"CGCGC"})


def test_every_misreading_gives_other_bytes_on_a_committed_case():
    kills = cc.killers()
    assert set(kills) == set(cc.WRONG_RULES) and all(kills[w] for w in cc.WRONG_RULES), kills


def test_the_grouped_matrices_are_the_single_ones():
    rng = np.random.default_rng(5)
    t = cc.rand_seq(rng, 90)
    reads = [cc.noisy(rng, t, 0.05, 0.05, 0.05) for _ in range(11)] + [b"", t]
    for r, D in zip(reads, cc.matrices(t, reads, group=4)):
        assert np.array_equal(D, cc.matrix(t, r))


def test_the_distances_are_those_of_editcheck_and_of_cf_edit_distances(eng):
    cc.check_independence(eng)


def test_the_literal_cases_on_the_device(eng):
    cc.check_literals(eng)


def test_template_lengths_around_the_wave_and_block_borders(eng):
    info = eng.consensus_info()
    assert (info["block_small"], info["block_big"], info["big_from"], info["k_ins"]) == (64, 256, 128, 4)
    positions = cc.border_positions((1, 63, 64, 65, 127, 128, 129, 300), info["max_len"])
    assert [len(t) for t, _ in positions] == [1, 63, 64, 65, 127, 128, 129, 300]
    for t, reads in positions[1:]:      # d = 0, and lengths that differ by exactly d, both ways
        d = [cc.one_pass(t, [r], 1000)[3][0] for r in reads[3:6]]
        assert d[0] == 0 and d[1] == len(t) - len(reads[4]) > 0 and d[2] == len(reads[5]) - len(t) > 0
    cc.check(eng, positions, 3)
    for p in positions:      # and each as a call of one position
        cc.check(eng, [p], 2)


def test_one_to_130_reads_per_position(eng):
    cc.check(eng, cc.many_reads_positions((1, 2, 63, 64, 65, 130)), 2)


def test_a_2055_base_position(eng):
    t, reads, truth = cc.workload_position(20261510)
    got = cc.check(eng, [(t, reads[:3])], 2)
    assert got[0][0][1:] == (3, 0)


def test_more_positions_than_the_launch_cap(eng):
    cc.check_more_positions_than_the_launch_cap(eng)


def test_batches_that_cut_through_one_positions_reads(eng):
    cc.check_batches(eng)
    with pytest.raises(DeviceError, match="out of range"):
        eng.set_param("cons_batch_bytes", -1)


def test_no_position_and_no_read(eng):
    assert cc.device(eng, [], 2) == [[], []]
    assert cc.device(eng, [(b"ACGT", [])], 2) == [[(b"ACGT", 0, 0)]] * 2
    assert cc.device(eng, [(b"", []), (b"", [b""])], 1) == [[(b"", 0, 0), (b"", 1, 0)]]


def test_a_string_above_the_maximum_is_refused(eng):
    cc.check_too_long(eng, DeviceError)


def test_each_refusal_leaves_the_context_and_the_last_results(eng):
    cc.check_refusals(eng, DeviceError)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    cc.check_hygiene(eng, DeviceError)


@pytest.mark.parametrize("order", ["rev", "rand"])
def test_other_lane_orders_give_the_same_bytes(order):
    """A missing barrier shows as other bytes when the emulator runs the lanes of a block in another order."""
    import subprocess
    code = ("import conscheck as cc\nfrom centroflye_amd import _lib\nfrom centroflye_amd.engine import Engine\n"
            f"e = Engine(0, _lib.load({os.path.join(ROOT, 'tests', 'emu', 'libcfhip_emu.so')!r}))\n"
            "cc.check_literals(e)\ncc.check(e, cc.border_positions((63, 129), 8192), 2)\ncc.check(e, cc.many_reads_positions((5,), 200), 2)\n")
    env = dict(os.environ, CF_EMU_ORDER=order, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_on_the_ubsan_build():
    import subprocess
    from centroflye_amd import _lib
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        cc.check_literals(e)
        cc.check(e, cc.border_positions((1, 64, 129), 8192), 2)
        e.set_param("cons_batch_bytes", 700)
        cc.check(e, cc.many_reads_positions((5,), 60), 2)
    finally:
        e.close()


# ---------------------------------------------------------------- the command line
def _cli(emu_lib, argv):
    session.reset()
    session._engine = Engine(0, emu_lib)
    old = sys.argv
    try:
        sys.argv = ["eltr_polisher.py"] + [str(a) for a in argv]
        runpy.run_path(SCRIPT, run_name="__main__")
    finally:
        sys.argv = old
        session.reset()


def _tree_args(report, tmp_path, fixture):
    import editcheck as ec
    unit = tmp_path / "unit.fasta"
    unit.write_text(">u\nACGT\n")
    return ["--read-placement", ec.placement_csv(fixture, str(tmp_path)), "--unit", unit, "--ncrf", report(fixture), "--outdir", tmp_path / "polishing"]


def test_the_stage_end_to_end_on_tiny_without_flye(emu_lib, report, tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path / "empty"))      # no flye anywhere
    args = _tree_args(report, tmp_path, "tiny")
    _cli(emu_lib, args + ["--polisher", "consensus", "--num-iters", 3, "--position-report", "--flye-bin", "/nonexistent/flye", "--error-mode", "raw",
                          "--num-threads", 3])
    out = str(tmp_path / "polishing")
    finals, rows = cc.check_tree(out, 3)
    assert len(rows) == 3 * 60 and any(r[5] for r in rows) and all(r[4] for r in rows)
    assert sorted(fn for fn in os.listdir(out) if not fn.startswith("pos_")) == sorted(
        ["consensus_report.tsv", "position_changes.csv", "report.txt"] + [f"final_sequence{h}_{i}.fasta" for h in ("", "_hpc") for i in (1, 2, 3)])


def test_a_missing_position_and_a_string_beyond_the_limit_exit_without_a_file(emu_lib, report, tmp_path):
    import json
    with open(os.path.join(ROOT, "tests", "golden", "tiny.json")) as f:
        placed = json.load(f)["read_positions"]["placed"]
    csv = tmp_path / "read_positions.csv"
    csv.write_text(placed[0] + "\n" + placed[1].split(" ")[0] + " 200\n")
    unit = tmp_path / "unit.fasta"
    unit.write_text(">u\nACGT\n")
    out = tmp_path / "polishing"
    args = ["--read-placement", csv, "--unit", unit, "--ncrf", report("tiny"), "--outdir", out, "--polisher", "consensus"]
    with pytest.raises(SystemExit) as ei:
        _cli(emu_lib, args + ["--num-iters", 2])
    assert ei.value.code not in (0, None) and "position " in str(ei.value.code) and " has no reads" in str(ei.value.code)
    gap = int(str(ei.value.code).split("position ")[1].split(" ")[0])
    assert 0 < gap < 200 and os.listdir(out) == []
    # a read beyond the device's limit: the export is all there is afterwards
    csv.write_text(placed[0] + "\n")
    _cli(emu_lib, args[:-2] + ["--max-pos", 3])
    fn = out / "pos_1" / "read_units.fasta"
    fn.write_text(fn.read_text() + ">long\n" + "A" * 8193 + "\n")
    from centroflye_amd import eltr_polisher
    session.reset()
    session._engine = Engine(0, emu_lib)
    try:
        import math
        import types
        pol = eltr_polisher.ELTR_Polisher(types.SimpleNamespace(unit=str(unit), ncrf=report("tiny"), outdir=str(out), read_placement=str(csv), min_pos=0,
                                                                  max_pos=3, num_iters=2))
        with pytest.raises(eltr_polisher.PolishingError, match="position 1 has a sequence of 8193 bases"):
            pol.run_consensus(pol.unit_filenames(pol.map_pos2read()))
    finally:
        session.reset()
    assert sorted(os.listdir(out)) == [f"pos_{p}" for p in range(4)] and sorted(os.listdir(out / "pos_1")) == ["median_read_unit.fasta", "read_units.fasta"]
    with pytest.raises(SystemExit):
        _cli(emu_lib, args + ["--consensus-max-divergence-permille", -1])

"""The built-in consensus polisher (cf_consensus.hip) on a real MI355X against the rule's plain-Python restatement
(tests/conscheck.py; tests/test_emu_consensus.py pins the restatement itself): the literal cases, template lengths 1 .. 129, 2 055 and the
longest string taken, one byte more refused, 1 .. 130 reads per position, more positions than a launch has workgroups, batches that
cut through one position's reads, the workload's own shape (2 055 bases, 32 reads at the generator's error rates, 4 iterations)
with its quality condition, the refusals and the scratch hygiene, and scripts/eltr_polisher.py --polisher consensus end to end
on the `tiny` and `hor2055` fixtures without a flye on PATH."""
import json
import os
import subprocess
import sys

import pytest

import conscheck as cc
import editcheck as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "eltr_polisher.py")
WORKLOAD_SEED = 20261510      # chosen on the CPU: the restatement alone gives the true unit at iteration 1 and repeats it


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_literal_cases(eng):
    for name, t, reads, permille, want in cc.LITERALS:
        assert [g[0] for g in cc.consensus(t, reads, len(want), permille)] == list(want), name
    cc.check_literals(eng)


def test_the_distances_are_those_of_editcheck_and_of_cf_edit_distances(eng):
    cc.check_independence(eng)


def test_template_lengths_around_the_wave_and_block_borders(eng):
    info = eng.consensus_info()
    assert (info["block_small"], info["block_big"], info["big_from"], info["k_ins"]) == (64, 256, 128, 4)
    positions = cc.border_positions((1, 63, 64, 65, 127, 128, 129), info["max_len"])
    assert [len(t) for t, _ in positions] == [1, 63, 64, 65, 127, 128, 129]
    cc.check(eng, positions, 3)
    for p in positions:      # and each as a call of one position
        cc.check(eng, [p], 2)


def test_a_template_of_2055_bases_and_one_of_the_longest_taken(eng):
    max_len = eng.consensus_info()["max_len"]
    positions = cc.border_positions((2055, max_len), max_len)
    assert [len(t) for t, _ in positions] == [2055, max_len] and max(len(r) for r in positions[1][1]) == max_len
    cc.check(eng, positions, 2)
    # at 1 000 permille the band of the longest pair may grow to every diagonal: the launch takes its largest LDS window
    cc.check(eng, [(positions[1][0], positions[1][1][:2])], 1, 1000)


def test_one_byte_above_the_maximum_is_refused(eng):
    from centroflye_amd.engine import DeviceError
    cc.check_too_long(eng, DeviceError)


def test_one_to_130_reads_per_position(eng):
    cc.check(eng, cc.many_reads_positions((1, 2, 63, 64, 65, 130)), 2)


def test_more_positions_than_the_launch_cap(eng):
    assert eng.consensus_info()["launch_cap"] >= 256
    cc.check_more_positions_than_the_launch_cap(eng)


def test_batches_that_cut_through_one_positions_reads(eng):
    cc.check_batches(eng)


def test_the_workloads_own_shape_and_its_quality(eng):
    t, reads, truth = cc.workload_position(WORKLOAD_SEED)
    assert len(truth) == 2055 and len(reads) == 32 and ec.nw(t, truth) > 50
    got = cc.check(eng, [(t, reads)], 4)
    assert [g[0] for g in got] == [(truth, 32, 0)] * 4      # iteration 1 is the true unit, iterations 2 - 4 repeat it
    ms = eng.consensus_info()["phase_ms"]
    assert ms["align"] > 0.0 and ms["total"] >= ms["align"]


def test_each_refusal_leaves_the_context_and_the_last_results(eng):
    from centroflye_amd.engine import DeviceError
    cc.check_refusals(eng, DeviceError)


def test_two_rounds_leave_the_same_live_bytes_and_the_same_results(eng):
    from centroflye_amd.engine import DeviceError
    cc.check_hygiene(eng, DeviceError)


def _run(args, tmp_path):
    empty = tmp_path / "no_flye_here"
    empty.mkdir(exist_ok=True)
    return subprocess.run([sys.executable, SCRIPT] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PATH=str(empty)))


@pytest.mark.parametrize("fixture", ["tiny", "hor2055"])
def test_the_stage_end_to_end_without_flye(report, tmp_path, fixture):
    unit = tmp_path / "unit.fasta"
    unit.write_text(">u\nACGT\n")
    out = tmp_path / "polishing"
    r = _run(["--read-placement", ec.placement_csv(fixture, str(tmp_path)), "--unit", unit, "--ncrf", report(fixture), "--outdir", out,
              "--polisher", "consensus", "--num-iters", 3, "--position-report"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    finals, rows = cc.check_tree(str(out), 3)
    assert len(rows) == 3 * {"tiny": 60, "hor2055": 16}[fixture] and all(r[4] for r in rows)
    assert sorted(fn for fn in os.listdir(out) if not fn.startswith("pos_")) == sorted(
        ["consensus_report.tsv", "position_changes.csv", "report.txt"] + [f"final_sequence{h}_{i}.fasta" for h in ("", "_hpc") for i in (1, 2, 3)])


def test_a_missing_position_exits_without_a_file(report, tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "tiny.json")) as f:
        placed = json.load(f)["read_positions"]["placed"]
    csv = tmp_path / "read_positions.csv"
    csv.write_text(placed[0] + "\n" + placed[1].split(" ")[0] + " 200\n")
    unit = tmp_path / "unit.fasta"
    unit.write_text(">u\nACGT\n")
    out = tmp_path / "polishing"
    r = _run(["--read-placement", csv, "--unit", unit, "--ncrf", report("tiny"), "--outdir", out, "--polisher", "consensus", "--num-iters", 2], tmp_path)
    assert r.returncode not in (0, None) and " has no reads" in r.stderr and "position " in r.stderr
    assert os.listdir(out) == []

"""scripts/eltr_polisher.py beyond the export, on the host-emulated kernels against the REFERENCE's recorded answers
(tests/golden/edit_cases.json: the reference's own read_polishing, compare_polished_sequences and export_results on the same
fabricated trees): --assemble-only on every golden tree, the full stage with a stub Flye that records its argument vector, the
export alone when no new flag is given, the line of a distance above --max-edit-distance, both error exits, --position-report."""
import json
import os
import runpy
import stat
import sys

import pytest

import editcheck as ec
from centroflye_amd import eltr_polisher, session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = ec.load_cases()
SCRIPT = os.path.join(ROOT, "scripts", "eltr_polisher.py")


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


def _args(pol):
    p = pol.params
    return ["--read-placement", p.read_placement, "--unit", p.unit, "--ncrf", p.ncrf, "--outdir", p.outdir]


def _results(outdir):
    return sorted(fn for fn in os.listdir(outdir) if not fn.startswith("pos_"))


@pytest.mark.parametrize("name", [t["name"] for t in ec.TREES if not t["gap"]])
def test_assemble_only_on_the_golden_trees(emu_lib, report, tmp_path, name):
    spec = next(t for t in ec.TREES if t["name"] == name)
    g = G["trees"][name]
    pol, files, made = ec.build_tree(spec, report(spec["fixture"]), str(tmp_path))
    assert made == g["inputs"], "the fabricated tree is not the recorded one"
    _cli(emu_lib, _args(pol) + ["--assemble-only", "--num-iters", spec["num_iters"]])
    outdir = pol.params.outdir
    with open(os.path.join(outdir, "report.txt")) as f:
        assert f.read() == g["report"]
    assert ec.digest_finals(outdir) == g["files"]
    assert _results(outdir) == sorted(list(g["files"]) + ["report.txt"])      # nothing else, no .tmp left
    with open(os.path.join(outdir, "final_sequence_1.fasta")) as f:
        lines = f.read().split("\n")
    assert lines[0] == ">polished_repeat_1" and len(lines) == 3 and len(lines[1]) == g["final_lengths"][0] and lines[2] == ""


def test_the_gap_tree_is_refused_as_the_reference_raises(emu_lib, report, tmp_path):
    spec = next(t for t in ec.TREES if t["gap"])
    g = G["trees"][spec["name"]]
    assert g["error"] == "KeyError"
    pol, files, made = ec.build_tree(spec, report(spec["fixture"]), str(tmp_path))
    assert made == g["inputs"] and ec.gap_position(pol.params.outdir) == g["gap_position"]
    del files[g["gap_position"]]
    session.reset()
    session._engine = Engine(0, emu_lib)
    try:
        with pytest.raises(eltr_polisher.PolishingError, match=f"position {g['gap_position']} has no reads"):
            pol.assemble(files)
    finally:
        session.reset()
    assert _results(pol.params.outdir) == []


STUB = '''#!{python}
import json, os, sys
a = sys.argv
with open({log!r}, "a") as f:
    f.write(json.dumps(a) + "\\n")
target, n, out = a[a.index("--polish-target") + 1], int(a[a.index("-i") + 1]), a[a.index("-o") + 1]
seq = "".join(ln.strip() for ln in open(target).read().splitlines()[1:])
for i in range(1, n + 1):
    s = seq if i == n else seq[:7 * i] + "T" + seq[7 * i + (i % 2):]
    with open(os.path.join(out, "polished_%d.fasta" % i), "w") as f:
        f.write(">contig_1\\n" + s + "\\n")
'''


def _small_run(report, tmp_path, far=None):
    """A placement of the first placed read of `tiny` alone (positions 0 .. its units), or with a second read far behind it."""
    with open(os.path.join(ROOT, "tests", "golden", "tiny.json")) as f:
        placed = json.load(f)["read_positions"]["placed"]
    csv = tmp_path / "read_positions.csv"
    lines = [placed[0]] + ([placed[1].split(" ")[0] + f" {far}"] if far is not None else [])
    csv.write_text("\n".join(lines) + "\n")
    unit = tmp_path / "unit.fasta"
    unit.write_text(">u\nACGT\n")
    return ["--read-placement", csv, "--unit", unit, "--ncrf", report("tiny"), "--outdir", tmp_path / "polishing"]


def test_the_full_stage_with_a_stub_flye(emu_lib, report, tmp_path):
    log = tmp_path / "flye_calls.jsonl"
    stub = tmp_path / "flye_stub"
    stub.write_text(STUB.format(python=sys.executable, log=str(log)))
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    args = _small_run(report, tmp_path) + ["--max-pos", 9]
    out = tmp_path / "polishing"
    # centroFlye.py's own command line (:227-250)
    _cli(emu_lib, args + ["--error-mode", "nano", "--num-iters", 3, "--num-threads", 5, "--flye-bin", stub, "--position-report"])
    positions = sorted(int(d[4:]) for d in os.listdir(out) if d.startswith("pos_"))
    assert positions == list(range(len(positions))) and len(positions) >= 5
    calls = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert calls == [[str(stub), "--nano-raw", str(out / f"pos_{p}" / "read_units.fasta"), "--polish-target",
                      str(out / f"pos_{p}" / "median_read_unit.fasta"), "-i", "3", "-t", "5", "-o", str(out / f"pos_{p}")] for p in positions]
    units = ["".join((out / f"pos_{p}" / "median_read_unit.fasta").read_text().splitlines()[1:]) for p in positions]
    finals = ["".join(u[:7 * i] + "T" + u[7 * i + (i % 2):] for u in units) for i in (1, 2)] + ["".join(units)]
    for i in (1, 2, 3):
        assert (out / f"final_sequence_{i}.fasta").read_text() == f">polished_repeat_{i}\n{finals[i - 1]}\n"
        assert (out / f"final_sequence_hpc_{i}.fasta").read_text() == f">polished_repeat_{i}\n{ec.hpc(finals[i - 1].encode()).decode()}\n"
    want = []
    for i in (1, 2):
        for what, f in (("polishing", lambda s: s), ("homopolymer compressed polishing", lambda s: ec.hpc(s.encode()).decode())):
            x, y = f(finals[i - 1]), f(finals[i])
            want += [f"Alignment {what} seq {i} vs {i + 1}:",
                     str({'editDistance': ec.nw(x.encode(), y.encode()), 'alphabetLength': len(set(x + y)), 'locations': [(None, len(y) - 1)], 'cigar': None})]
    assert (out / "report.txt").read_text().splitlines() == want
    # position_changes.csv: iteration position distance
    rows = [ln.split(" ") for ln in (out / "position_changes.csv").read_text().splitlines()]
    assert [(int(r[0]), int(r[1])) for r in rows] == [(i, p) for i in (1, 2) for p in positions]
    pol = {p: [(u[:7 * i] + "T" + u[7 * i + (i % 2):]) for i in (1, 2)] + [u] for p, u in zip(positions, units)}
    assert [int(r[2]) for r in rows] == [ec.nw(pol[p][i - 1].encode(), pol[p][i].encode()) for i in (1, 2) for p in positions]
    assert len({r[2] for r in rows}) > 1

    # the defaults of the new flags are the reference's (:174-177); --polish selects the full stage without --num-iters
    log.write_text("")
    os.environ["PATH"], old = str(tmp_path / "bin") + os.pathsep + os.environ["PATH"], os.environ["PATH"]
    try:
        (tmp_path / "bin").mkdir()
        (tmp_path / "bin" / "flye").write_text(stub.read_text())
        (tmp_path / "bin" / "flye").chmod(stub.stat().st_mode)
        _cli(emu_lib, args + ["--polish"])
    finally:
        os.environ["PATH"] = old
    calls = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert os.path.basename(calls[0][0]) == "flye" and calls[0][1] == "--nano-raw" and calls[0][5:9] == ["-i", "4", "-t", "16"] and len(calls) == len(positions)
    assert (out / "final_sequence_4.fasta").exists()


def test_without_a_new_flag_the_export_is_all(emu_lib, report, tmp_path):
    args = _small_run(report, tmp_path)
    for flags in ([], ["--export-only"], ["--export-only", "--num-iters", 2]):
        _cli(emu_lib, args + flags)
        out = tmp_path / "polishing"
        assert _results(out) == [] and sorted(os.listdir(out / "pos_0")) == ["median_read_unit.fasta", "read_units.fasta"]


def test_a_distance_above_the_limit(emu_lib, report, tmp_path, capsys):
    spec = ec.TREES[0]
    g = G["trees"][spec["name"]]
    pol, files, made = ec.build_tree(spec, report(spec["fixture"]), str(tmp_path))
    want = g["report"].splitlines()
    dists = [int(ln.split("'editDistance': ")[1].split(",")[0]) for ln in want[1::2]]
    limit = sorted(dists)[len(dists) // 2]          # some comparisons at or below it, some above
    assert min(dists) <= limit < max(dists)
    capsys.readouterr()
    _cli(emu_lib, _args(pol) + ["--assemble-only", "--num-iters", spec["num_iters"], "--max-edit-distance", limit])
    err = capsys.readouterr().err
    got = (tmp_path / spec["name"] / "report.txt").read_text().splitlines()
    assert got[0::2] == want[0::2]
    n_over = 0
    for d, ln, ref in zip(dists, got[1::2], want[1::2]):
        if d <= limit:
            assert ln == ref
        else:
            assert ln == str({'editDistance': -1, 'alphabetLength': 4, 'locations': None, 'cigar': None})
            n_over += 1
    assert n_over >= 1 and err.count("--max-edit-distance") == n_over and f"more than {limit} places" in err
    assert ec.digest_finals(pol.params.outdir) == g["files"]           # the sequences do not depend on the limit


def test_the_error_exits_leave_no_partial_output(emu_lib, report, tmp_path):
    spec = dict(ec.TREES[0], num_iters=2)
    pol, files, made = ec.build_tree(spec, report(spec["fixture"]), str(tmp_path))
    outdir = pol.params.outdir
    missing = os.path.join(outdir, "pos_7", "polished_2.fasta")
    os.remove(missing)
    with pytest.raises(SystemExit) as ei:
        _cli(emu_lib, _args(pol) + ["--assemble-only", "--num-iters", 2, "--position-report"])
    assert ei.value.code not in (0, None) and missing in str(ei.value.code)
    assert _results(outdir) == []
    # a position without reads inside the range: a second read placed far behind the first
    args = _small_run(report, tmp_path, far=200)
    _cli(emu_lib, args)
    out = tmp_path / "polishing"
    positions = sorted(int(d[4:]) for d in os.listdir(out) if d.startswith("pos_"))
    gap = next(p for p in range(positions[0], positions[-1]) if p not in positions)
    for p in positions:
        for i in (1, 2):
            (out / f"pos_{p}" / f"polished_{i}.fasta").write_text(">c\nACGT\n")
    with pytest.raises(SystemExit) as ei:
        _cli(emu_lib, args + ["--assemble-only", "--num-iters", 2])
    assert ei.value.code not in (0, None) and f"position {gap} " in str(ei.value.code)
    assert _results(out) == []
    # and a Flye that fails
    with pytest.raises(SystemExit) as ei:
        _cli(emu_lib, _small_run(report, tmp_path) + ["--num-iters", 2, "--flye-bin", "false"])
    assert ei.value.code not in (0, None) and _results(out) == []

"""scripts/map_reads.py on the host-emulated kernels against the REFERENCE's recorded answers: the fixture's own
read_positions.csv (the golden's lines) as the backbone, every read mapped, and --only-unplaced on `lowcov`, whose greedy run
leaves three reads as `None`."""
import os
import runpy
import sys

import pytest

import mapcheck
from centroflye_amd import session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in mapcheck.load_cases()["cases"]}


def _run(emu_lib, report, golden, tmp_path, name, min_unit, only_unplaced=False):
    g = golden(name)
    placement = tmp_path / "read_positions.csv"
    placement.write_text("\n".join(g["read_positions"]["placed"] + g["read_positions"]["none"]) + "\n")
    out = tmp_path / "out"
    argv = ["map_reads.py", "--ncrf", report(name), "--genomic-kmers", os.path.join(ROOT, "tests", "golden", f"{name}.unique_kmers.txt"),
            "--read-placement", str(placement), "--outdir", str(out), "--min-unit", str(min_unit)] + (["--only-unplaced"] if only_unplaced else [])
    session.reset()
    session._engine = Engine(0, emu_lib)
    old = sys.argv
    try:
        sys.argv = argv
        runpy.run_path(os.path.join(ROOT, "scripts", "map_reads.py"), run_name="__main__")
    finally:
        sys.argv = old
        session.reset()
    assert os.listdir(out) == ["mapped_positions.csv"]      # written through .tmp and a rename
    return (out / "mapped_positions.csv").read_text().splitlines(), g


def _want(case, r_id):
    v = case["expect"]["reads"][r_id]
    return f"{r_id} None" if v is None else f"{r_id} {v[0]} {v[1]} {v[2]}"


@pytest.mark.parametrize("name", ["tiny", "hor2055", "lowcov"])
@pytest.mark.parametrize("min_unit", [5, 2])
def test_mapped_positions_of_every_read_equal_the_reference(emu_lib, report, golden, tmp_path, name, min_unit):
    lines, g = _run(emu_lib, report, golden, tmp_path, name, min_unit)
    case = CASES[f"{name}_full_t{min_unit}_10"]
    from centroflye_amd import _host
    ids = _host.parse_report(report(name)).ids
    assert [ln.split(" ")[0] for ln in lines] == list(ids)      # one line per query read, in report order
    assert lines == [_want(case, r_id) for r_id in ids]
    assert any(not ln.endswith(" None") for ln in lines)


def test_only_unplaced_maps_the_none_tail_of_lowcov(emu_lib, report, golden, tmp_path):
    lines, g = _run(emu_lib, report, golden, tmp_path, "lowcov", 5, only_unplaced=True)
    none = [ln.split(" ")[0] for ln in g["read_positions"]["none"]]
    assert len(none) == 3
    case = CASES["lowcov_full_t5_10"]
    assert sorted(ln.split(" ")[0] for ln in lines) == sorted(none)
    assert sorted(lines) == sorted(_want(case, r_id) for r_id in none)
    assert all(not ln.endswith(" None") for ln in lines)      # the reference's map_reads_fast places all three

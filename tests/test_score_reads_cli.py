"""scripts/map_reads.py --exact / --check-exact / --rescore-placed on the host-emulated kernels against the REFERENCE's recorded
answers (tests/golden/score_reads_cases.json): `hor2055` with its own read_positions.csv (the golden's lines) as the backbone,
thresholds (5, 10), under which the fast mapper leaves 15 of the 39 reads unmapped and the exact one keeps 26.  Without the flags
the output directory holds what it held before."""
import os
import runpy
import sys

import mapcheck
import scorecheck
from centroflye_amd import _host, session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = scorecheck.load_cases()
CASE = next(c for c in ALL["cases"] if c["name"] == "hor2055_full_t5_10")


def _run(emu_lib, report, golden, tmp_path, flags):
    g = golden("hor2055")
    placement = tmp_path / "read_positions.csv"
    placement.write_text("\n".join(g["read_positions"]["placed"] + g["read_positions"]["none"]) + "\n")
    out = tmp_path / "out"
    argv = ["map_reads.py", "--ncrf", report("hor2055"), "--genomic-kmers", os.path.join(ROOT, "tests", "golden", "hor2055.unique_kmers.txt"),
            "--read-placement", str(placement), "--outdir", str(out), "--min-unit", "5"] + flags
    session.reset()
    session._engine = Engine(0, emu_lib)
    old = sys.argv
    try:
        sys.argv = argv
        runpy.run_path(os.path.join(ROOT, "scripts", "map_reads.py"), run_name="__main__")
    finally:
        sys.argv = old
        session.reset()
    return {fn: (out / fn).read_text().splitlines() for fn in sorted(os.listdir(out))}


def _none(p):
    return "None" if p < 0 else str(p)


def test_the_three_flags_against_the_golden(emu_lib, report, golden, tmp_path):
    files = _run(emu_lib, report, golden, tmp_path, ["--exact", "--check-exact", "--rescore-placed"])
    # every file is written through .tmp and a rename
    assert list(files) == ["mapped_positions.csv", "mapped_positions_exact.csv", "mapping_disagreements.csv", "placement_scores.csv"]
    ids = list(_host.parse_report(report("hor2055")).ids)
    rows = dict(zip(CASE["read_ids"], CASE["reads"]))
    fast = {r: (tuple(v) if v is not None else None) for r, v in CASE["fast"].items()}
    assert files["mapped_positions.csv"] == [f"{r} None" if fast[r] is None else f"{r} {fast[r][0]} {fast[r][1]} {fast[r][2]}" for r in ids]
    # map_reads with threshold (5, 10): the reference's verdict of every read, in report order
    want = [f"{r} {_none(rows[r][16])} {rows[r][17]} {rows[r][18]}" if rows[r][15] else f"{r} None" for r in ids]
    assert files["mapped_positions_exact.csv"] == want
    assert sum(1 for ln in want if not ln.endswith(" None")) == 26
    # debug: the mapped reads whose exact answer under the same thresholds over the same range is another one
    want = [f"{r} {fast[r][0]} {fast[r][1]} {fast[r][2]} {_none(rows[r][0])} {rows[r][1]} {rows[r][2]}"
            for r in ids if fast[r] is not None and list(fast[r]) != rows[r][0:3]]
    assert files["mapping_disagreements.csv"] == want and len(want) == 24
    # every placed read at its own position under (0, 0), against the numpy statement (pinned to the same golden by the emulator suite)
    g = golden("hor2055")
    placed = {ln.split(" ")[0]: int(ln.split(" ")[1]) for ln in g["read_positions"]["placed"]}
    session.reset()
    session._engine = Engine(0, emu_lib)
    try:
        got_ids, unit_ptr, cloud_ptr, entries = mapcheck.Sources(session._engine, report, ALL).use("hor2055")
    finally:
        session.reset()
    assert got_ids == ids
    row = {r: i for i, r in enumerate(ids)}
    c = scorecheck.contig(unit_ptr, cloud_ptr, entries, [row[r] for r in placed], list(placed.values()), 2)
    want = []
    for r in ids:
        if r in placed:
            p, s0, s1 = scorecheck.score_read(unit_ptr, cloud_ptr, entries, c, row[r], placed[r], placed[r], 0, 0)
            assert p == placed[r]
            want.append(f"{r} {p} {s0} {s1}")
    assert files["placement_scores.csv"] == want and len(want) == len(placed) > 30
    assert sum(1 for ln in want if ln.endswith(" 0 0")) < len(want) // 4      # placed reads agree with their contig


def test_without_the_flags_the_output_is_what_it_was(emu_lib, report, golden, tmp_path):
    files = _run(emu_lib, report, golden, tmp_path, [])
    assert list(files) == ["mapped_positions.csv"]
    fast = CASE["fast"]
    ids = list(_host.parse_report(report("hor2055")).ids)
    assert files["mapped_positions.csv"] == [f"{r} None" if fast[r] is None else f"{r} {fast[r][0]} {fast[r][1]} {fast[r][2]}" for r in ids]

"""centroflye_amd.debruijn_graph.polish, the drop-in for the reference's ``polish``: with a stub in Flye's place it writes and prints
what the reference wrote and printed for the same inputs (tests/golden/mono_polish_cases.json, captured by
tools/capture_mono_polish_cases.py), byte for byte; with polisher='consensus' (on the emulator) the export is the same, every
polished_k.fasta is conscheck.consensus on the exported strings, and the three TSVs are supportcheck's restatement; and wherever it
refuses, no file is left."""
import contextlib
import io
import json
import os

import pytest

import conscheck as cc
import monopolishcheck as mp
import supportcheck as sc
from centroflye_amd import debruijn_graph as dg
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "mono_polish_cases.json")) as f:
    GOLDEN = json.load(f)
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_golden_cases_are_those_of_the_check_module():
    assert [{k: v for k, v in c.items() if k not in ("files", "printed")} for c in CASES] == json.loads(json.dumps(mp.polish_cases()))
    assert len(CASES) >= 12


@pytest.mark.parametrize("x", range(len(CASES)), ids=lambda x: CASES[x]["name"][:40])
def test_with_a_stub_in_flyes_place_the_files_and_the_command_lines_are_the_references(x, tmp_path):
    case = CASES[x]
    flye = mp.write_flye_stub(str(tmp_path))
    outdir = str(tmp_path / "work" / "polishing")
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert dg.polish(*mp.inputs(case), outdir, case["n_iter"], case["n_threads"], flye_bin=flye) is None
    assert mp.tree_texts(outdir) == case["files"]
    assert mp.printed_record(printed.getvalue(), outdir, flye) == case["printed"]


def test_the_reverse_complement_is_the_references_table():
    assert dg.RC("ATGCatgc-NnRx") == "xRnN-gcatGCAT"


def test_the_consensus_polisher_on_the_golden_inputs(eng, tmp_path):
    for x, case in enumerate(CASES):
        outdir = str(tmp_path / f"c{x}" / "polishing")
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            dg.polish(*mp.inputs(case), outdir, case["n_iter"], case["n_threads"], flye_bin="/nonexistent/flye", polisher="consensus", engine=eng)
        assert printed.getvalue() == ""
        got = mp.tree_texts(outdir)
        exported = {fn: text for fn, text in case["files"].items() if fn.endswith(("reads.fasta", "template.fasta"))}
        assert {fn: got[fn] for fn in exported} == exported
        want = sc.polish_tree_expected(exported, case["n_iter"])
        assert set(got) == set(exported) | set(want), case["name"]
        for fn in want:
            assert got[fn] == want[fn], (case["name"], fn)
        # the polished files against conscheck itself
        for fn in exported:
            if fn.endswith("template.fasta"):
                d = fn[:-len("template.fasta")]
                t = exported[fn].split("\n")[1].encode().upper()
                reads = [r.encode().upper() for r in exported[d + "reads.fasta"].split("\n")[1::2]]
                for k, (out, _, _) in enumerate(cc.consensus(t, reads, case["n_iter"]), 1):
                    assert got[d + f"polished_{k}.fasta"].split("\n")[1] == out.decode(), (case["name"], fn, k)
        assert not [fn for fn in got if fn.endswith(".tmp")]


def _one_unit(reads_of_unit):
    reads = {"ra": "ACGTTGCAAC" * 6, "rb": "ACGTTGCAAC" * 6, "rc": "ACGTTGCATC" * 6}
    monomers = {"mA": "ACGTTG", "mB": "CAACAA", "mA'": "x", "mB'": "x"}
    return ["ABa", "B"], [[(0, 1), (2, 2)], [(0, 0)]], [[{("ra", 0): (0, 29, "+"), ("rb", 0): (2, 33, "-")}, reads_of_unit], [{("rc", 1): (5, 40, "+")}]], reads, monomers


def _nothing_left(tmp_path):
    return not os.path.exists(tmp_path / "polishing") and os.listdir(tmp_path) == []


def test_an_uncovered_pseudounit_is_refused_and_named(eng, tmp_path):
    for kw in (dict(polisher="consensus", engine=eng), dict(flye_bin="sh")):
        with pytest.raises(dg.PolishError, match="pseudounit 1 of scaffold 0 .*covered by no read"):
            dg.polish(*_one_unit({}), str(tmp_path / "polishing"), 2, 1, **kw)
        assert _nothing_left(tmp_path)


def test_uncovered_monomers_fills_the_unit_from_its_letters(eng, tmp_path):
    out = str(tmp_path / "polishing")
    dg.polish(*_one_unit({}), out, 2, 1, polisher="consensus", uncovered="monomers", engine=eng)
    got = mp.tree_texts(out)
    assert got["scaffold_0/pseudounit_1/template.fasta"] == ">s_0_t_1_monomers\n" + dg.RC("ACGTTG") + "\n" and got["scaffold_0/pseudounit_1/reads.fasta"] == ""
    assert got["scaffold_0/pseudounit_1/polished_2.fasta"] == ">consensus_s_0_t_1_iter_2\n" + dg.RC("ACGTTG") + "\n"
    exported = {fn: text for fn, text in got.items() if fn.endswith(("reads.fasta", "template.fasta"))}
    want = sc.polish_tree_expected(exported, 2)
    assert {fn: got[fn] for fn in want} == want
    rows = [ln.split("\t") for ln in got["consensus_report.tsv"].splitlines()]
    assert rows[0][-1] == "uncovered" and [r[-1] for r in rows[1:]] == ["0", "1", "0"] and rows[2][2] == "0"
    assert got["scaffold_0/scaffold_0.support.tsv"].splitlines()[-1].split("\t")[1:] == ["1", "0", "0"]
    assert got["scaffold_0/scaffold_0.fasta"].split("\n")[1].endswith(dg.RC("ACGTTG"))


def test_a_missing_read_a_long_string_and_a_missing_flye_leave_no_file(eng, tmp_path):
    out = str(tmp_path / "polishing")
    with pytest.raises(dg.PolishError, match="the read 'nobody' is not among the reads"):
        dg.polish(*_one_unit({("nobody", 0): (0, 5, "+")}), out, 2, 1, polisher="consensus", engine=eng)
    assert _nothing_left(tmp_path)
    args = list(_one_unit({("long", 0): (0, 8192, "+")}))
    args[3] = dict(args[3], long="A" * 9000)
    assert eng.consensus_info()["max_len"] == 8192
    with pytest.raises(dg.PolishError, match="pseudounit 1 of scaffold 0 has a sequence of 8193 bases"):
        dg.polish(*args, out, 2, 1, polisher="consensus", engine=eng)
    assert _nothing_left(tmp_path)
    with pytest.raises(dg.PolishError, match="Flye binary '/nonexistent/flye' was not found"):
        dg.polish(*_one_unit({("ra", 0): (0, 9, "+")}), out, 2, 1, flye_bin="/nonexistent/flye")
    assert _nothing_left(tmp_path)
    # a Flye that leaves no polished_N.fasta: everything written so far goes again
    with pytest.raises(dg.PolishError, match="Flye left no "), contextlib.redirect_stdout(io.StringIO()):
        dg.polish(*_one_unit({("ra", 0): (0, 9, "+")}), out, 2, 1, flye_bin="true")
    assert _nothing_left(tmp_path)
    with pytest.raises(ValueError):
        dg.polish(*_one_unit({}), out, 2, 1, polisher="medaka")
    assert _nothing_left(tmp_path)

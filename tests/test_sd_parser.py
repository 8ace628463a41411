"""centroflye_amd/sd_parser.py (SD_Report, MonoString, get_stats) against the reference's scripts/sd_parser.py on the captured cases
of tests/golden/sd_parser_cases.json (tools/capture_sd_parser_cases.py ran the reference's module on them): key by key, the order
of the reads, mono2nucl with its order, the strand, the name maps and get_stats; then the parser on the built-in decomposer's own
output (through the host emulator), the MonoString methods, and the command line."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import monodeccheck as mc
from centroflye_amd import sd_parser
from centroflye_amd.sd_parser import MonoString, SD_Report, get_ngap_symbols, get_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "sd_parser_cases.json")) as f:
    CASES = json.load(f)["cases"]


def report_of(case, tmp_path):
    fa, rep = tmp_path / "monomers.fasta", tmp_path / "decomposition.tsv"
    fa.write_text(case["monomers_fasta"])
    rep.write_text(case["tsv"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # (the reference warns on an all-gap read: the mean of nothing; this parser has no need to)
        return SD_Report(str(rep), str(fa), max_gap=case["max_gap"])


def test_the_cases_cover_what_they_must():
    assert len(CASES) >= 40
    names = " ".join(c["name"] for c in CASES)
    for what in ("primed monomers", "exactly 0.5", "leading, trailing and inner", "100 and of 101", "x.5", "all-gap", "interleaved", "27 monomers"):
        assert what in names, what
    reads = [r for c in CASES for r in c["reads"]]
    assert sum(r[2] == "-" for r in reads) >= 20 and sum(r[1] == "" for r in reads) >= 3 and sum("?" in r[1] for r in reads) >= 20
    assert not any(r[0].isdigit() for r in reads)
    assert all(len(c["names_map"]) == 2 * min(26, c["monomers_fasta"].count(">")) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_golden_case(case, tmp_path):
    rep = report_of(case, tmp_path)
    assert list(rep.monostrings) == [r[0] for r in case["reads"]]      # the order of the reads too
    for r_id, string, strand, m2n in case["reads"]:
        ms = rep.monostrings[r_id]
        assert ms.name == r_id and ms.tostring() == string and ms.string == list(string) and ms.strand == strand and len(ms) == len(string)
        assert [[c, m, st, en] for c, (m, st, en) in ms.mono2nucl.items()] == m2n
        assert all(isinstance(v, int) for _, (_, st, en) in ms.mono2nucl.items() for v in (st, en))
        ms.assert_validity()
    assert list(rep.monomer_names_map.items()) == [tuple(x) for x in case["names_map"]]
    assert list(rep.rev_monomer_names_map.items()) == [tuple(x) for x in case["rev_names_map"]]
    stats = get_stats(rep.monostrings)
    assert list(stats) == ["ntranslations", "min_len", "max_len", "mean_len", "tot_len", "ngaps", "pgaps", "ngap_runs"]
    assert {k: (float(v) if k in ("mean_len", "pgaps") else int(v)) for k, v in stats.items()} == case["stats"]
    assert get_ngap_symbols(rep.monostrings) == case["stats"]["ngaps"]


def test_a_monomer_past_the_26th_has_no_letter(tmp_path):
    case = next(c for c in CASES if "27 monomers" in c["name"])
    bad = dict(case, tsv=case["tsv"] + "r27\tm26_x\t900\t905\t90.00\t+\n")
    with pytest.raises(KeyError):
        report_of(bad, tmp_path)
    rep = report_of(case, tmp_path)
    assert "m26_x" not in rep.monomer_names_map and rep.monomer_names_map["m25_x"] == "Z" and rep.monomer_names_map["m25_x'"] == "z"


def test_ids_stay_strings(tmp_path):
    """the documented difference: the reference's CSV reader turns all-numeric ids into integers"""
    case = dict(CASES[0], tsv="".join("7\t" + ln.split("\t", 1)[1] + "\n" for ln in CASES[0]["tsv"].splitlines()[:3]))
    assert list(report_of(case, tmp_path).monostrings) == ["7"]


def test_monostring_methods():
    ms = MonoString("r")
    for c, st, en in (("A", 0, 9), ("b", 10, 19)):
        ms.add_monomer(c, st, en)
    ms.add_gap(2)
    ms.add_monomer("C", 40, 49)
    assert ms.tostring() == "Ab??C" and len(ms) == 5 and ms[1] == "b" and ms[1:4] == "b??" and ms.strand == "+"
    ms[2] = "X"
    assert ms.tostring() == "AbX?C"
    ms[2:4] = "??"
    assert ms.string == list("Ab??C")
    ms[2:4] = ["?", "?"]
    ms.check_reverse()      # 1 of 3 letters is lower case
    assert ms.strand == "+" and ms.mono2nucl == {0: ("A", 0, 9), 1: ("b", 10, 19), 4: ("C", 40, 49)}
    ms.trim_read(1, 5)
    assert ms.tostring() == "b??C" and ms.mono2nucl == {0: ("b", 10, 19), 3: ("C", 40, 49)}
    ms.trim_read(0, 3)
    ms.strip()
    assert ms.tostring() == "b" and ms.mono2nucl == {0: ("b", 10, 19)}
    ms.check_reverse()
    assert ms.strand == "-" and ms.tostring() == "B" and ms.mono2nucl == {0: ("B", 19, 10)}
    other = MonoString("s", string=ms.string, mono2nucl=ms.mono2nucl)
    other.add_gap(1)
    assert ms.tostring() == "B" and other.tostring() == "B?"      # copies
    assert not hasattr(MonoString, "split")      # belongs to the error-correction follow-up


def test_the_parser_on_the_decomposers_own_output(emu_lib, tmp_path):
    from centroflye_amd import _host
    from centroflye_amd.engine import Engine
    rng = np.random.default_rng(91)
    monomers = [(b"mn%d" % k, mc.rand_seq(rng, n)) for k, n in enumerate((33, 41, 37))]
    seqs = [s for _, s in monomers]
    reads = [(b"own_%d" % q, mc.rc(b"".join(seqs[k] for k in ks)) if q & 1 else b"".join(seqs[k] for k in ks))
             for q, ks in enumerate(([0, 1, 2, 0], [2, 0, 1], [1, 1, 2, 0, 1]))]
    planted = ["ABCA", "CAB", "BBCAB"]
    with Engine(0, emu_lib) as e:
        flat = b"".join(r for _, r in reads)
        off = np.concatenate([[0], np.cumsum([len(r) for _, r in reads])]).astype(np.int64)
        info, ptr, inst = e.monodec(seqs, flat, off)
    n = _host.write_sd_report(str(tmp_path / "d.tsv"), [x for x, _ in reads], [x for x, _ in monomers], info, ptr, inst)
    assert n == 12 and sorted(os.listdir(tmp_path)) == ["d.tsv"]
    mc.write_fasta(tmp_path / "m.fasta", monomers)
    rep = SD_Report(str(tmp_path / "d.tsv"), str(tmp_path / "m.fasta"))
    assert [(k, ms.tostring(), ms.strand) for k, ms in rep.monostrings.items()] == [("own_%d" % q, planted[q], "+-"[q & 1]) for q in range(3)]
    ms = rep.monostrings["own_1"]
    assert ms.mono2nucl[0] == ("C", 110, 74) and ms.mono2nucl[2] == ("B", 40, 0)      # (monomer.swapcase(), en, st) of the turned read


def test_the_command_line_prints_the_statistics(tmp_path):
    case = CASES[2]
    (tmp_path / "m.fasta").write_text(case["monomers_fasta"])
    (tmp_path / "d.tsv").write_text(case["tsv"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sd_parser.py"), "-i", str(tmp_path / "d.tsv"), "-m", str(tmp_path / "m.fasta")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    s = case["stats"]
    assert r.stdout.splitlines() == [
        f"Number of translations: {s['ntranslations']}", f"Min length = {s['min_len']}", f"Mean length = {s['mean_len']}",
        f"Max length = {s['max_len']}", f"Total length = {s['tot_len']}", f"#(%) Gap symbols = {s['ngaps']} ({s['pgaps']})",
        f"#Gap runs = {s['ngap_runs']}"]
    # the flat import the reference's scripts use
    code = "import sd_parser; print(sd_parser.SD_Report.__module__, sd_parser.MonoString.__name__, callable(sd_parser.get_stats))"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "scripts"), capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["centroflye_amd.sd_parser", "MonoString", "True"], r.stderr

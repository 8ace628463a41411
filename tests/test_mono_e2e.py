"""scripts/centroFlyeMono.py end to end on the host emulator: a generated String Decomposer report of 36 D6Z1-shaped reads from a
planted array with one variant monomer and unreliable instances -> corrected monostrings -> contigs, both files equal to what the
reference's modules make of the same report (tests/golden/mono_graph_cases.json, "e2e"); and the refusal without --stop-after."""
import os
import subprocess
import sys

import pytest

import monographcheck as gc
from centroflye_amd import session
from centroflye_amd.engine import Engine
from test_mono_graph import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


def test_end_to_end_tsv_to_contigs(emu_session, tmp_path):
    gc.check_end_to_end(tmp_path, GOLDEN["e2e"])


def test_stop_after_correction_writes_the_monostrings_only(emu_session, tmp_path):
    from centroflye_amd import centroflye_mono
    fasta, tsv, _ = gc.e2e_inputs(dict(gc.E2E, n_reads=3, read_units=4, array_units=6, variant=(2, 7, "C")))
    (tmp_path / "m.fasta").write_text(fasta)
    (tmp_path / "d.tsv").write_text(tsv)
    assert centroflye_mono.main(["--sd-report", str(tmp_path / "d.tsv"), "--monomers", str(tmp_path / "m.fasta"), "--centromeric-reads", "none",
                                 "--outdir", str(tmp_path / "o"), "--stop-after", "correction"]) == 0
    assert os.listdir(tmp_path / "o") == ["ec_monostrings.tsv"]
    lines = (tmp_path / "o" / "ec_monostrings.tsv").read_text().splitlines()
    assert len(lines) == 3 and all(len(line.split("\t")) == 4 for line in lines) and {line.split("\t")[2] for line in lines} == {"+", "-"}


def test_without_stop_after_it_refuses_and_writes_nothing(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "centroFlyeMono.py"), "--sd-report", "x.tsv", "--monomers", "m.fasta",
                        "--centromeric-reads", "r.fasta", "--outdir", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, None) and "not built" in r.stderr and "--stop-after" in r.stderr
    assert os.listdir(tmp_path) == []

"""The cen6 driver's polishing stage end to end on the host emulator (scripts/centroFlyeMono.py --stop-after polishing --polisher
consensus): a decomposition report, monomers and reads of a planted nucleotide array (tests/monopolishcheck.py) in, polishing/ out,
checked against the restatement on the exported files and against the planted array.  tests/test_gpu_mono_polish_e2e.py runs the
same on the hardware."""
import pytest

import monopolishcheck as mp
from centroflye_amd import centroflye_mono, session
from centroflye_amd.engine import Engine


@pytest.fixture()
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


def test_from_the_report_to_the_polished_scaffold(emu_session, tmp_path):
    figures = mp.check_end_to_end(tmp_path, centroflye_mono.main)
    assert figures["units"] >= 20


def test_a_refusal_of_polish_exits_non_zero_and_leaves_no_polishing_directory(emu_session, tmp_path):
    import contextlib
    import io
    import os
    mp.write_e2e_inputs(str(tmp_path))
    with open(tmp_path / "reads.fasta", "w") as f:      # the reads the report speaks of are not in the file
        f.write(">somebody_else\nACGT\n")
    with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
        centroflye_mono.main(mp.e2e_args(str(tmp_path), "polishing"))
    assert e.value.code not in (0, None) and "is not among the reads" in str(e.value.code)
    out = tmp_path / "out_polishing"
    assert os.path.isfile(out / "read_pseudounits.tsv") and not os.path.exists(out / "polishing")
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(io.StringIO()):
        centroflye_mono.main(mp.e2e_args(str(tmp_path), "polishing") + ["--consensus-max-divergence-permille", "-1"])
    assert e.value.code not in (0, None)


def test_the_stages_and_the_refusal_without_stop_after(tmp_path):
    assert centroflye_mono.STAGES[-1] == "polishing" and centroflye_mono.STAGES[-2] == "pseudounits"
    args = [a for a in mp.e2e_args(str(tmp_path), "polishing")]
    x = args.index("--stop-after")
    with pytest.raises(SystemExit) as e:
        centroflye_mono.main(args[:x] + args[x + 2:])
    assert all(w in str(e.value.code) for w in ("polishing", "not built", "--stop-after")) and list(tmp_path.iterdir()) == []

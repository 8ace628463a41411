"""The sketch sweep cut at d*(a) (knob dist_sketch_tail) on the host-emulated kernels: the cases of tests/sketchtailcheck.py, each with
the knob at 1 and at 0, against the plain restatement; and, on the -DCF_DIST_DIAG_COUNT build, the sums of the useful items and of
all items that the work-list builder reports.  tests/test_gpu_dist_sketch_tail.py runs the same cases on an MI355X."""
import os
import re
import subprocess
import sys

import pytest

import sketchtailcheck as stc
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(dist_slots=2048, dist_block=128)      # (a small distance kernel: the emulator's time per launch goes with its threads and LDS)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    for name, value in BASE.items():
        e.set_param(name, value)
    yield e
    e.close()


@pytest.mark.parametrize("params", stc.PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_core_reads_under_the_stage_parameters(engine, params):
    """min_cov 1 (no sketch), 2 and 4; max_d below the long read, below every read and beyond all; min_d 2."""
    stc.run(engine, stc.case("core", **params))


@pytest.mark.parametrize("min_cov", [2, 4])
def test_posting_lists_of_16_17_64_and_65(engine, min_cov):
    stc.run(engine, stc.case("postings", min_cov=min_cov))


@pytest.mark.parametrize("layout", list(stc.LAYOUTS))
def test_core_reads_in_the_other_layouts(engine, layout):
    stc.run(engine, stc.case("core"), stc.LAYOUTS[layout])


def test_core_reads_with_a_table_that_splits(engine):
    st = stc.run(engine, stc.case("core", min_cov=2), dict(dist_slots=256))
    assert st["n_spilled"] > 0


def test_a_repeated_rank_in_a_row_switches_the_cut_off(engine):
    stc.run_repeated_rank(engine)


def test_generator_reads_through_the_exchange_path(emu_lib, tmp_path):
    stc.run_exchange(emu_lib, str(tmp_path / "rdv"), BASE)


DIAG = r"""
import sys
root, lib_path, what, tail = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [root, root + "/tests"]
import pathcheck, shapecheck, sketchtailcheck as stc
from centroflye_amd import _lib
from centroflye_amd.engine import Engine
e = Engine(0, _lib.load(lib_path))
e.set_param("dist_slots", 2048); e.set_param("dist_block", 128); e.set_param("dist_sketch_tail", tail)
if what == "repeated":
    pathcheck.check_clouds(e, *stc.repeated_rank_clouds(), 1, 150, 4, 0.8)
else:
    c = stc.case(what)
    e.load_arrays(*shapecheck.to_arrays(c["reads"], c["units"]))
    e.count_kmers(c["k"]); e.select_rare(c["max_nonuniq"], c["lo"], c["hi"]); e.build_clouds()
    shapecheck._check_dist(e, c, c["naive"], what)
print("DIAG-OK")
"""


@pytest.fixture(scope="module")
def diag_lib(emu_lib):
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh"), "diag_count", "-DCF_DIST_DIAG_COUNT"])
    return os.path.join(ROOT, "tests", "emu", "libcfhip_emu_diag_count.so")


def _sums(diag_lib, what, tail):
    r = subprocess.run([sys.executable, "-c", DIAG, ROOT, diag_lib, what, str(tail)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIAG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.findall(r"sketch items=(\d+) of items=(\d+) \(rows are sets=(\d)\)", r.stderr)
    assert len(m) == 1, r.stderr[-2000:]
    return tuple(int(x) for x in m[0])


def test_the_builder_reports_fewer_sketch_items_than_items_only_where_it_may(diag_lib):
    """Core reads: tail items exist with the knob at 1, none at 0.  A repeated rank in one row: every item useful."""
    n_a, n, sets = _sums(diag_lib, "core", 1)
    assert sets == 1 and 0 < n_a < n
    assert _sums(diag_lib, "core", 0) == (n, n, 1)
    n_a, n, sets = _sums(diag_lib, "repeated", 1)
    assert sets == 0 and n_a == n > 0

"""First k-mers with equal posting lists swept once (knob dist_classes) on the host-emulated kernels: the cases of tests/classcheck.py,
each with the knob at 1 and at 0, against the plain restatement; and, on the -DCF_DIST_DIAG_COUNT build, the numbers of classes and
members that the launch reports.  tests/test_gpu_dist_classes.py runs the same cases on an MI355X."""
import os
import re
import subprocess
import sys

import pytest

import classcheck as cc
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


@pytest.mark.parametrize("min_cov", [1, 2, 4])
def test_classes_of_2_and_3_members_that_select_each_other_and_near_misses(engine, min_cov):
    cc.run(engine, cc.case("core", min_cov=min_cov))


@pytest.mark.parametrize("bits", [1, 3])
def test_different_lists_with_one_hash_are_not_merged(engine, bits):
    """One or three hash bits: the six different lists that begin in unit 0 of read 0 collide; the comparison of the lists decides."""
    cc.run(engine, cc.case("core"), dict(dist_class_bits=bits))
    cc.run(engine, cc.case("big"), dict(dist_class_bits=bits))


def test_a_run_of_equal_lists_longer_than_the_member_cap(engine):
    st = cc.run(engine, cc.case("big"))
    assert st["n_dist_passes"] < len(cc.case("big")["naive"]["kmers"])


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_core_reads_in_the_other_layouts(engine, layout):
    cc.run(engine, cc.case("core"), cc.LAYOUTS[layout])


def test_a_class_whose_table_splits(engine):
    st = cc.run(engine, cc.case("big", min_cov=2), dict(dist_slots=256))
    assert st["n_spilled"] > 0


@pytest.mark.parametrize("min_cov", [2, 4])
def test_rows_of_a_class_across_edge_chunks_with_marked_slot_sweep_and_in_scan_filter(engine, min_cov):
    cc.run(engine, cc.case("rows", min_cov=min_cov), cc.TIGHT)
    cc.run(engine, cc.case("rows", min_cov=min_cov), dict(dist_edge_chunk=16))


def test_edge_cap_below_the_rows(engine):
    cc.run(engine, cc.case("rows"), edge_cap=50)
    cc.run(engine, cc.case("rows"), cc.TIGHT, edge_cap=50)


def test_two_partitions_split_the_members_of_one_list(engine):
    c = cc.case("core")
    both = [g for g in c["classes"] if len({x % 2 for x in g}) == 2]
    assert both, "a list whose k-mers fall into both partitions"
    cc.run(engine, c, n_parts=2)
    cc.run(engine, cc.case("big"), n_parts=2)


@pytest.mark.parametrize("doubled", [True, False])
def test_a_repeated_rank_in_a_row_switches_the_classes_off(engine, doubled):
    """The results with a class of 2 next to a doubled rank, and of the same clouds as sets (the diagnostic build's test shows which of the
    two launches formed the class)."""
    cc.run_repeated_rank(engine, doubled)


def test_generator_reads_through_the_exchange_path(emu_lib, tmp_path):
    cc.run_exchange(emu_lib, str(tmp_path / "rdv"), BASE)


DIAG = r"""
import sys
root, lib_path, what, on = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [root, root + "/tests"]
import pathcheck, shapecheck, sketchtailcheck as stc, classcheck as cc
from centroflye_amd import _lib
from centroflye_amd.engine import Engine
e = Engine(0, _lib.load(lib_path))
e.set_param("dist_slots", 2048); e.set_param("dist_block", 128); e.set_param("dist_classes", on)
if what in ("repeated", "repeated_as_sets"):
    cc.run_repeated_rank(e, what == "repeated")
else:
    cc.run(e, cc.case(what), classes=(on,))
print("DIAG-OK")
"""


@pytest.fixture(scope="module")
def diag_lib(emu_lib):
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh"), "diag_count", "-DCF_DIST_DIAG_COUNT"])
    return os.path.join(ROOT, "tests", "emu", "libcfhip_emu_diag_count.so")


def _counts(diag_lib, what, on):
    r = subprocess.run([sys.executable, "-c", DIAG, ROOT, diag_lib, what, str(on)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIAG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.findall(r"classes=(\d+) members=(\d+)", r.stderr)
    assert len(m) == 1, r.stderr[-2000:]
    return tuple(int(x) for x in m[0])


def test_the_launch_reports_its_classes_and_members(diag_lib):
    """A hash collision may lose a merge, never make one: no fewer classes than the equal lists cut at the cap.  Knob 0 and clouds
    whose rows are not sets: every first k-mer its own class."""
    for what in ("core", "big"):
        least, members = cc.capped_classes(cc.case(what)["naive"])
        classes, m = _counts(diag_lib, what, 1)
        assert m == members and least <= classes < members, (what, least, classes, m, members)
        assert _counts(diag_lib, what, 0) == (members, members)
    # cf_set_clouds: the clouds with the class (0, 2) as sets form it; with rank 1 twice in a row the launch forms none, because the switch fired
    least, members = cc.prove_repeated_rank_clouds()
    classes, m = _counts(diag_lib, "repeated_as_sets", 1)
    assert m == members and least <= classes < members, (least, classes, m, members)
    assert _counts(diag_lib, "repeated", 1) == (members, members)

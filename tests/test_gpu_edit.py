"""cf_edit_distances / cf_hpc on a real MI355X against the REFERENCE's recorded answers (tests/golden/edit_cases.json): every
case of the emulator suite and the ones of hardware size — a whole 2 055-base HOR unit deleted and inserted, two unrelated
strings of 20 000 bases, one pair just below and one just above the kernel's own LDS/HBM switch point, homopolymer runs longer
than a scan tile — and scripts/eltr_polisher.py --assemble-only end to end on the golden trees."""
import os
import subprocess
import sys

import numpy as np
import pytest

import editcheck as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = ec.load_cases()


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def singles(eng):
    info = eng.edit_info()
    assert {k: info[k] for k in G["shape"]} == G["shape"], "the goldens straddle other borders than the kernel's: regenerate them"
    return ec.single_cases(info["lane_bytes"], info["turn_bytes"])


def test_every_single_case_alone_and_as_one_batch(eng, singles):
    assert {"hor2055_unit_deleted", "hor2055_unit_inserted", "ident", "ident_mismatch_99999"} <= {c[0] for c in singles}
    ec.check_singles(eng, G, singles)


def test_every_pair_of_start_offsets_mod_8(eng):
    for name, data, a_off, b_off, a, b in ec.offset_cases():
        d, _ = eng.edit_distances(data, a_off, b_off)
        assert int(d[0]) == G["offsets"][name]["distance"], name


def test_unrelated_strings_and_both_sides_of_the_switch_point(eng):
    lds_diags = eng.edit_info()["lds_diags"]
    cases = ec.switch_cases(lds_diags) + ec.big_cases()
    assert len(cases[0][1]) + 1 <= lds_diags < len(cases[1][1]) + 1
    ec.check_singles(eng, G, cases)
    name, a, b = cases[0]
    w = G["single"][name]["distance"]
    assert ec.one_pair(eng, a, b, w) == w and ec.one_pair(eng, a, b, w - 1) == -1
    # the same pairs with the wavefronts forced into HBM, and into LDS arrays of a few diagonals next to HBM ones
    for forced in (1, 4096):
        with eng.knobs(edit_lds_diags=forced):
            ec.check_singles(eng, G, cases[1:])


def test_the_limit(eng, singles):
    ec.check_limits(eng, G, [c for c in singles if c[0] in ("len_65_65", "len_0_9", "len_64_0", "empty_empty", "ident", "ident_mismatch_0",
                                                              "hor171_unit_deleted", "hor2055_unit_inserted", "related_1200", "N_and_case")])


def test_batches_of_none_one_and_three_thousand(eng):
    d, ms = eng.edit_distances(b"", [0], [0])
    assert d.size == 0 and ms == 0.0
    data, a_off, b_off = ec.batch_case()
    assert ec.sha(data) == G["batch"]["sha"]
    d, _ = eng.edit_distances(data, a_off[:2], b_off[:2])
    assert d.tolist() == G["batch"]["distances"][:1]
    d, ms = eng.edit_distances(data, a_off, b_off)
    assert d.tolist() == G["batch"]["distances"] and ms > 0.0
    d, _ = eng.edit_distances(data, a_off, b_off, 3)
    assert d.tolist() == [w if w <= 3 else -1 for w in G["batch"]["distances"]]


def test_hpc_with_runs_longer_than_a_tile_and_the_resident_bytes(eng):
    for key, long_runs in (("hpc_short", False), ("hpc_long", True)):
        data, off, seqs = ec.hpc_case(long_runs)
        out, out_off = eng.hpc(data, off)
        assert ec.sha(out) == G[key]["sha_out"] and np.diff(out_off).tolist() == G[key]["lengths"]
        assert eng.edit_info()["resident_bytes"] == len(data) + out.size
    # many tiles, runs across every tile border: 3 MB of runs of 1 .. 40 000 equal bytes
    rng = np.random.default_rng(7)
    runs = rng.integers(1, 40001, 150)
    sym = np.frombuffer(b"ACGT", np.uint8)[np.arange(150) % 4]
    data = np.repeat(sym, runs)
    off = np.array([0, 5, 5, int(runs[:70].sum()) + 3, data.size], np.int64)
    out, out_off = eng.hpc(data, off)
    want = [ec.hpc(data[off[i]:off[i + 1]].tobytes()) for i in range(4)]
    assert out.tobytes() == b"".join(want) and np.diff(out_off).tolist() == [len(w) for w in want]
    every = np.concatenate([off, off[-1] + out_off[1:]])
    d, _ = eng.edit_distances(None, every[4:-1], every[5:], 1000)
    assert d.tolist() == [ec.nw(x, y) for x, y in zip(want[:-1], want[1:])]


@pytest.mark.parametrize("name", [t["name"] for t in ec.TREES if not t["gap"]])
def test_assemble_only_end_to_end_on_the_golden_trees(report, tmp_path, name):
    spec = next(t for t in ec.TREES if t["name"] == name)
    g = G["trees"][name]
    pol, files, made = ec.build_tree(spec, report(spec["fixture"]), str(tmp_path))
    assert made == g["inputs"]
    p = pol.params
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "eltr_polisher.py"), "--read-placement", p.read_placement, "--unit", p.unit,
           "--ncrf", p.ncrf, "--outdir", p.outdir, "--assemble-only", "--num-iters", str(spec["num_iters"]), "--position-report"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(p.outdir, "report.txt")) as f:
        assert f.read() == g["report"]
    assert ec.digest_finals(p.outdir) == g["files"]
    with open(os.path.join(p.outdir, "position_changes.csv")) as f:
        rows = [ln.split(" ") for ln in f.read().splitlines()]
    assert len(rows) == (spec["num_iters"] - 1) * len(files) and all(0 <= int(r[2]) <= 12 for r in rows)

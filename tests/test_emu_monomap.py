"""Monoreads mapped to the graph's edges (cf_monomap.hip: cf_monomap_run / _get / _info) on the host emulator.  The reference has only a
Python loop behind the rule, so the rule's plain-Python restatement (tests/monomapcheck.py) is first pinned: literal cases with every
hit, path and flag written out, and eight planted misreadings that each change a literal.  Then the kernels are compared with it,
every field: every k of the issue's list, k against the string lengths, the edge letters, the read letters and the hits on the
borders of the block and of the tiles, more reads than a launch has threads, a long run on one edge, every refusal with the live
bytes as they were, and two calls in a row.  The shapes of hardware size are in tests/test_gpu_monomap.py."""
import os
import subprocess
import sys

import pytest

import monomapcheck as mc
from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


# ---------------------------------------------------------------- pinning the restatement (CPU only)
def test_the_literal_cases_pin_the_restatement():
    assert len(mc.LITERALS) >= 16
    for case in mc.LITERALS:
        assert mc.check_literal(*case), case[0]
    # every literal result is written out in full: a hit holds the read window's letters at its place in its edge, the hits ascend,
    # the path is the hits' edges with equal neighbours collapsed
    for name, edges, uv, reads, k, want in mc.LITERALS:
        assert len(want) == len(reads) and len(uv) == len(edges)
        for read, (hits, path, valid) in zip(reads, want):
            assert all(edges[e][j:j + k] == read[i:i + k] and len(read[i:i + k]) == k for e, j, i in hits)
            assert [i for _, _, i in hits] == sorted({i for _, _, i in hits})
            assert path == [e for x, e in enumerate(h[0] for h in hits) if x == 0 or hits[x - 1][0] != e]
            assert valid == all(uv[a][1] == uv[b][0] for a, b in zip(path, path[1:]))
    names = " | ".join(c[0] for c in mc.LITERALS)
    for what in ("twice in one edge", "once in each of two edges", "only in the reads", "only in the edges", "hit, miss, hit", "A-B-A", "self-loop",
                 "invalid join", "first hit of the next", "beside a gap", "behind gaps", "shorter than k", "empty reads", "E = 0", "R = 0", "k = 1"):
        assert what in names, what


def test_every_misreading_changes_a_literal():
    kills = mc.killers()
    assert set(kills) == set(mc.WRONG_RULES) and len(mc.WRONG_RULES) == 8 and all(kills[w] for w in mc.WRONG_RULES), kills


# ---------------------------------------------------------------- device == restatement
def test_the_literal_cases_on_the_device(eng):
    mc.check_literals(eng)


def test_small_seeded_graphs(eng):
    mc.check_small_seeded(eng)


def test_every_k_no_round_one_round_the_overlap_and_powers_of_two(eng):
    assert mc.ALL_K == (1, 2, 3, 5, 8, 9, 255, 256, 257)
    mc.check_all_k(eng, n_edge_letters=900, n_read_letters=1100)
    info = eng.monomap_info()
    assert info["k"] == 257 and info["n_rounds"] == 9


def test_k_against_the_string_lengths(eng):
    mc.check_lengths_against_k(eng)


def test_letters_and_hits_on_the_borders_of_block_and_tile(eng):
    info = eng.monomap_info()
    assert (info["block"], info["sort_tile"], info["scan_tile"]) == (256, 2048, 2048)
    mc.check_borders(eng, (255, 256, 257, 2047, 2048, 2049))


def test_more_reads_than_a_launch_has_threads(eng):
    info = eng.monomap_info()
    n = info["launch_cap"] * info["block"]
    assert n <= 1 << 14
    mc.check_many_reads(eng, n + 5)


def test_a_long_run_on_one_edge(eng):
    mc.check_long_run(eng, 5000)


def test_the_numpy_restatement_agrees_with_the_dict(eng):
    """what the large shapes of the GPU suite are compared with"""
    import numpy as np
    rng = np.random.default_rng(3)
    for k, n_edge_letters, letters in ((1, 20, b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"), (2, 300, b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"), (3, 400, b"ABCDEFGH"), (8, 400, b"ABCD")):
        edges, uv, reads = mc.graph_like(rng, n_edge_letters, 500, 3, 6, letters)
        want = mc.restate(edges, uv, reads, k)
        hits, n_hits, n_path, valid, path = mc.restate_np(edges, uv, reads, k)
        assert [tuple(h) for h in hits.tolist()] == [(r,) + h for r, (hl, _, _) in enumerate(want) for h in hl]
        assert n_hits.tolist() == [len(h) for h, _, _ in want] and n_path.tolist() == [len(p) for _, p, _ in want]
        assert valid.tolist() == [v for _, _, v in want] and path.tolist() == [e for _, p, _ in want for e in p]
        assert len(hits) > 20 and not all(valid)
        mc.check_np(eng, edges, uv, reads, k)


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    mc.check_refusals(eng, DeviceError)


def test_two_calls_leave_the_same_live_bytes_and_touch_no_times_or_stats(eng):
    mc.check_hygiene(eng)


def test_get_before_any_run_is_refused(emu_lib):
    e = Engine(0, emu_lib)
    try:
        mc.check_get_before_run(e, DeviceError)
    finally:
        e.close()


@pytest.mark.parametrize("order", ["rev", "rand"])
def test_other_lane_orders_give_the_same_results(order):
    code = ("import monomapcheck as mc\nfrom centroflye_amd import _lib\nfrom centroflye_amd.engine import Engine\n"
            f"e = Engine(0, _lib.load({os.path.join(ROOT, 'tests', 'emu', 'libcfhip_emu.so')!r}))\n"
            "mc.check_literals(e)\nmc.check_small_seeded(e, 12)\nmc.check_borders(e, (257, 2049))\n")
    env = dict(os.environ, CF_EMU_ORDER=order, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]

"""Exact counts of gap-free windows of monostrings (cf_monokmers.hip: cf_monokmers_run / _get / _info) on the host emulator.  The
reference has only a Python loop behind the rule, so the rule's plain-Python restatement (tests/monokmercheck.py) is first pinned:
literal cases with every k-mer, count, first position and occurrence list written out, and seven planted misreadings that each
change a literal.  Then the kernels are compared with it, every field: every k of the issue's list, k against the string lengths,
gaps at and beside a window's ends, N on the borders of the sort's tile and of the streaming passes' block, more strings than a
launch has threads, min_mult on both sides of a count, every refusal with the live bytes as they were, two calls in a row, and
the same under UndefinedBehaviorSanitizer.  The shapes of hardware size are in tests/test_gpu_monokmers.py."""
import os
import subprocess
import sys

import pytest

import monokmercheck as mc
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
    # every literal result is written out in full: the lists hold `count` windows, ascending, the first one first
    for name, strings, k, mm, want in mc.LITERALS:
        for kmer, count, first, occ in want:
            assert len(kmer) == k and count == len(occ) >= mm and occ[0] == first and occ == sorted(occ)
            assert all(strings[s][i:i + k] == kmer for s, i in occ)
        assert [f for _, _, f, _ in want] == sorted(f for _, _, f, _ in want)


def test_every_misreading_changes_a_literal():
    kills = mc.killers()
    assert set(kills) == set(mc.WRONG_RULES) and len(mc.WRONG_RULES) == 7 and all(kills[w] for w in mc.WRONG_RULES), kills


# ---------------------------------------------------------------- device == restatement
def test_the_literal_cases_on_the_device(eng):
    mc.check_literals(eng)


def test_small_seeded_strings(eng):
    mc.check_small_seeded(eng)


def test_every_k_no_round_one_round_the_overlap_and_powers_of_two(eng):
    assert mc.ALL_K == (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257)
    mc.check_all_k(eng, n_strings=3, n_letters=420)
    info = eng.monokmers_info()
    assert info["k"] == 257 and info["n_rounds"] == 9


def test_k_against_the_string_lengths(eng):
    mc.check_lengths_against_k(eng)


def test_n_on_the_borders_of_block_and_tile(eng):
    info = eng.monokmers_info()
    assert (info["block"], info["sort_tile"], info["scan_tile"]) == (256, 2048, 2048)
    mc.check_borders(eng, (255, 256, 257, 2047, 2048, 2049))


def test_more_strings_than_a_launch_has_threads(eng):
    info = eng.monokmers_info()
    n = info["launch_cap"] * info["block"]
    assert n <= 1 << 14
    mc.check_many_strings(eng, n + 5)


def test_two_alphabets_of_ids_wider_than_a_byte(eng):
    """more than 256 distinct pairs, so the ids of round 2 need their second byte"""
    import numpy as np
    rng = np.random.default_rng(3)
    strings = mc.random_strings(rng, 4, 900, bytes(range(65, 91)), 0.01)
    mc.check(eng, strings, 4, 1)
    assert eng.monokmers_info()["n_distinct"] > 256
    mc.check(eng, strings, 3, 2)


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    mc.check_refusals(eng, DeviceError)


def test_two_calls_leave_the_same_live_bytes_and_touch_no_times_or_stats(eng):
    mc.check_hygiene(eng)


def test_get_before_any_run_is_refused(emu_lib):
    e = Engine(0, emu_lib)
    try:
        import ctypes as C
        n = C.c_int64()
        with pytest.raises(DeviceError, match="no cf_monokmers_run before"):
            e._check(e._lib.cf_monokmers_get(e._ctx, None, 0, C.byref(n), None, None, 0, None), "cf_monokmers_get")
        first = e.monokmers([b"ABAB"], 2, 1)
        assert first.tolist() == [(0, 0, 2, 0), (0, 1, 1, 1)]
        with pytest.raises(DeviceError, match="kept no positions"):
            e._check(e._lib.cf_monokmers_get(e._ctx, None, 0, None, (C.c_int64 * 3)(), None, 0, None), "cf_monokmers_get")
    finally:
        e.close()


@pytest.mark.parametrize("order", ["rev", "rand"])
def test_other_lane_orders_give_the_same_results(order):
    code = ("import monokmercheck as mc\nfrom centroflye_amd import _lib\nfrom centroflye_amd.engine import Engine\n"
            f"e = Engine(0, _lib.load({os.path.join(ROOT, 'tests', 'emu', 'libcfhip_emu.so')!r}))\n"
            "mc.check_literals(e)\nmc.check_small_seeded(e, 12)\nmc.check_borders(e, (257, 2049))\n")
    env = dict(os.environ, CF_EMU_ORDER=order, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_on_the_ubsan_build():
    from centroflye_amd import _lib
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")], env=dict(os.environ, CF_EMU_UBSAN="1"))
    e = Engine(0, _lib.load(os.path.join(ROOT, "tests", "emu", "libcfhip_emu_ubsan.so")))
    try:
        mc.check_literals(e)
        mc.check_small_seeded(e, 12)
        mc.check_lengths_against_k(e)
        mc.check_borders(e, (255, 2049))
        mc.check_hygiene(e)
    finally:
        e.close()

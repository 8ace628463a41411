"""Exact counts of gap-free windows of monostrings (cf_monokmers.hip) on a real MI355X against the rule's plain-Python restatement
(tests/monokmercheck.py; tests/test_emu_monokmers.py pins the restatement itself): the literal cases, every k of the issue's list,
k against the string lengths, N on the borders of the block and of the sort's and the scan's tiles (asserted from
cf_monokmers_info), more strings than a launch has threads, one string of 200 000 equal letters, more than 65 536 and more than
2^20 distinct k-mers, min_mult on both sides of a count, every refusal, and the scratch hygiene."""
import numpy as np
import pytest

import monokmercheck as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_literal_cases(eng):
    for case in mc.LITERALS:
        assert mc.check_literal(*case), case[0]
    mc.check_literals(eng)


def test_small_seeded_strings(eng):
    mc.check_small_seeded(eng)


def test_every_k_no_round_one_round_the_overlap_and_powers_of_two(eng):
    assert mc.ALL_K == (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257)
    mc.check_all_k(eng)


def test_k_against_the_string_lengths(eng):
    mc.check_lengths_against_k(eng)


def test_n_on_the_borders_of_block_and_tile(eng):
    info = eng.monokmers_info()
    assert (info["block"], info["sort_tile"], info["scan_tile"]) == (256, 2048, 2048)
    tile = info["sort_tile"]
    mc.check_borders(eng, (255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 1))


def test_more_strings_than_a_launch_has_threads(eng):
    info = eng.monokmers_info()
    n = info["launch_cap"] * info["block"]
    assert info["launch_cap"] >= 256 and n <= 1 << 20
    mc.check_many_strings(eng, n + 5)


def test_one_string_of_200000_equal_letters(eng):
    first, ptr, occ = eng.monokmers([b"A" * 200000, b"?", b"AAA"], 3, 1, True)
    assert first.tolist() == [(0, 0, 199999, 0)] and ptr.tolist() == [0, 199999]
    assert np.array_equal(occ["s"], np.r_[np.zeros(199998, np.int32), [2]]) and np.array_equal(occ["i"], np.r_[np.arange(199998, dtype=np.int32), [0]])
    info = eng.monokmers_info()
    assert (info["n_windows"], info["n_distinct"], info["n_rounds"]) == (199999, 1, 2)
    first = eng.monokmers([b"A" * 200000], 257, 2)
    assert first.tolist() == [(0, 0, 200000 - 256, 0)]


def test_more_than_65536_distinct_kmers(eng):
    rng = np.random.default_rng(5)
    strings = [rng.integers(65, 91, 30000, dtype=np.uint8).tobytes() for _ in range(5)]
    mc.check_np(eng, strings, 6, 1, 1 << 16)
    first = mc.check_np(eng, strings, 4, 2, 1 << 16)
    assert len(first) > 1000 and first["count"].min() == 2


def test_more_than_2_to_the_20_distinct_kmers(eng):
    rng = np.random.default_rng(6)
    strings = [rng.integers(65, 91, 300000, dtype=np.uint8).tobytes() for _ in range(4)]
    strings[1] = strings[1][:150000] + b"?" + strings[0][:100000] + b"?" + strings[1][150000:]      # planted repeats
    first = mc.check_np(eng, strings, 6, 1, 1 << 20)
    assert first["count"].max() >= 2
    first = mc.check_np(eng, strings, 6, 2, 1 << 20)
    assert len(first) >= 99000


def test_min_mult_against_counts_of_exactly_min_mult(eng):
    strings = [b"AB" * 7 + b"?" + b"CD" * 6, b"CD?AB"]
    for mm in (1, 6, 7, 8, 9):
        want = mc.check(eng, strings, 2, mm)
        counts = {kmer: c for kmer, c, _, _ in want}
        assert counts.get(b"AB") == (8 if mm <= 8 else None) and counts.get(b"CD") == (7 if mm <= 7 else None)
        assert counts.get(b"BA") == (6 if mm <= 6 else None)


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    from centroflye_amd.engine import DeviceError
    mc.check_refusals(eng, DeviceError)


def test_two_calls_leave_the_same_live_bytes_and_touch_no_times_or_stats(eng):
    mc.check_hygiene(eng)

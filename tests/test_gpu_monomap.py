"""Monoreads mapped to the graph's edges (cf_monomap.hip) on a real MI355X against the rule's plain-Python restatement
(tests/monomapcheck.py; tests/test_emu_monomap.py pins the restatement itself): the literal cases, every k of the issue's list, k
against the string lengths, the edge letters, the read letters and the hits on the borders of the block and of the sort's and the
scan's tiles (asserted from cf_monomap_info), more reads than a launch has threads, a read of 200 000 equal letters, more than 2^20
hits in one call, every refusal, and the scratch hygiene."""
import numpy as np
import pytest

import monomapcheck as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_get_before_any_run_is_refused():
    from centroflye_amd.engine import DeviceError, Engine
    with Engine(0) as e:
        mc.check_get_before_run(e, DeviceError)


def test_the_literal_cases(eng):
    for case in mc.LITERALS:
        assert mc.check_literal(*case), case[0]
    mc.check_literals(eng)


def test_small_seeded_graphs(eng):
    mc.check_small_seeded(eng)


def test_every_k_no_round_one_round_the_overlap_and_powers_of_two(eng):
    assert mc.ALL_K == (1, 2, 3, 5, 8, 9, 255, 256, 257)
    mc.check_all_k(eng)


def test_k_against_the_string_lengths(eng):
    mc.check_lengths_against_k(eng)


def test_letters_and_hits_on_the_borders_of_block_and_tile(eng):
    info = eng.monomap_info()
    assert (info["block"], info["sort_tile"], info["scan_tile"]) == (256, 2048, 2048)
    tile = info["sort_tile"]
    mc.check_borders(eng, (255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 1))


def test_more_reads_than_a_launch_has_threads(eng):
    info = eng.monomap_info()
    n = info["launch_cap"] * info["block"]
    assert info["launch_cap"] >= 256 and n <= 1 << 20
    mc.check_many_reads(eng, n + 5)


def test_a_read_of_200000_equal_letters(eng):
    mc.check_long_run(eng, 200000)


def test_more_than_2_to_the_20_hits_in_one_call(eng):
    rng = np.random.default_rng(6)
    edges, uv, reads = mc.graph_like(rng, 200000, 1300000, 5, 50, gap_rate=0.001, sub_rate=0.002, piece=3000)
    stats = mc.check_np(eng, edges, uv, reads, 6)
    assert stats["n_hits"] > 1 << 20 and stats["n_path"] > 100 and stats["n_indexed"] > 150000


def test_each_refusal_leaves_the_context_and_the_live_bytes(eng):
    from centroflye_amd.engine import DeviceError
    mc.check_refusals(eng, DeviceError)


def test_two_calls_leave_the_same_live_bytes_and_touch_no_times_or_stats(eng):
    mc.check_hygiene(eng)

"""The support of every emitted byte and the per-read results of the consensus polisher (cf_consensus_support, cf_consensus_reads) on
a real MI355X against the rule's plain-Python restatement (tests/supportcheck.py; tests/test_emu_support.py pins the restatement
itself): the same checks as on the emulator."""
import pytest

import supportcheck as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from centroflye_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_the_literal_cases(eng):
    sc.check_literals_pin_the_restatement()
    sc.check_literals(eng)


def test_template_lengths_1_to_5_and_around_64(eng):
    positions = sc.length_positions()
    sc.check(eng, positions, 2)
    for p in positions:
        sc.check(eng, [p], 1)


@pytest.mark.parametrize("slots", [255, 256, 257])
def test_global_slot_counts_around_the_vote_block(eng, slots):
    sc.check(eng, sc.slot_count_positions(slots), 2)


def test_more_positions_than_the_launch_cap(eng):
    assert eng.consensus_info()["launch_cap"] >= 256
    sc.check_more_positions_than_the_launch_cap(eng)


def test_many_small_batches(eng):
    sc.check_batches(eng)


def test_two_and_three_iterations_keep_their_own_support(eng):
    sc.check_iterations_keep_their_own_support(eng)


def test_200_random_positions(eng):
    got = sc.check(eng, sc.random_positions(), 2)
    assert sum(len(g[1]) for g in got[0]) == sum(len(g[0]) for g in got[0]) > 5000


def test_refusals_leave_the_last_run(eng):
    sc.check_refusals(eng)

"""The support of every emitted byte and the per-read results of the consensus polisher (cf_consensus_support, cf_consensus_reads) on
the host emulator.  The rule's restatement (tests/supportcheck.py, on conscheck.matrices and conscheck.walk) is first pinned by
hand-written cases with the expected `agree` written out and shown to be told from four misreadings by them; then the kernels
are compared with it entry by entry, and cf_consensus_get's outputs with conscheck.expected on the same inputs.  The same checks
run on the hardware in tests/test_gpu_support.py."""
import pytest

import conscheck as cc
import supportcheck as sc
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def eng(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def test_the_literal_cases_pin_the_restatement():
    sc.check_literals_pin_the_restatement()
    names = {c[0] for c in sc.LITERALS}
    assert len(names) == len(sc.LITERALS) >= 12


def test_every_misreading_gives_another_agree_on_a_literal_case():
    kills = sc.killers()
    assert set(kills) == set(sc.WRONG_RULES) and all(kills[w] for w in sc.WRONG_RULES), kills


def test_the_literal_cases_on_the_device(eng):
    sc.check_literals(eng)


def test_template_lengths_1_to_5_and_around_64(eng):
    positions = sc.length_positions()
    assert [len(t) for t, _ in positions] == [1, 2, 3, 4, 5, 63, 64, 65]
    sc.check(eng, positions, 2)
    for p in positions:
        sc.check(eng, [p], 1)


@pytest.mark.parametrize("slots", [255, 256, 257])
def test_global_slot_counts_around_the_vote_block(eng, slots):
    sc.check(eng, sc.slot_count_positions(slots), 2)


def test_more_positions_than_the_launch_cap(eng):
    sc.check_more_positions_than_the_launch_cap(eng)


def test_many_small_batches(eng):
    sc.check_batches(eng)


def test_two_and_three_iterations_keep_their_own_support(eng):
    sc.check_iterations_keep_their_own_support(eng)


def test_200_random_positions(eng):
    positions = sc.random_positions()
    assert len(positions) == 200 and max(len(t) for t, _ in positions) <= 96 and max(len(rs) for _, rs in positions) <= 9
    got = sc.check(eng, positions, 2)
    assert sum(len(g[1]) for g in got[0]) == sum(len(g[0]) for g in got[0]) > 5000
    assert any(0 < a < g[2] for g in got[0] for a in g[1]) and any(not v for g in got[0] for v in g[5])


def test_refusals_leave_the_last_run(eng):
    sc.check_refusals(eng)

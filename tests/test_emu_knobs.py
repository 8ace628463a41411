"""The distance stage's knobs and its dominance test on the host emulator (tests/emu), each against the oracle.

The knobs of cf_set_param that no deterministic test set before are set here, one setting at a time (with the knobs that make
their path matter), on the lowcov fixture at max_distance 2 and on hand-made clouds (pathcheck.tie_clouds: pairs that meet a threshold exactly and
one count short of it; pathcheck.check_synthetic_clouds: a posting list longer than a chunk).  Knobs named elsewhere:
dist_slots, dist_block, dist_sketch, dist_wide, dist_regions, dist_region_bytes, dist_dbits, dist_hot_cap, dist_post_atomics,
dist_edge_chunk, dist_stage, dist_sketch_bits, count_mode, count_bits and the place_* knobs in test_emu_kernels.py; dist_wgs and
place_chunk in test_gpu_parity.py / test_gpu_fullsize.py; comm_round_bytes and comm_self_p2p in test_gpu_parity.py (the exchange
on one rank, tests/sharded_worker.py).  The same matrix on a real MI355X: test_gpu_knobs.py."""
import pytest

import pathcheck
from centroflye_amd.engine import Engine

THRESHOLDS = (0.5, 0.6, 0.75, 0.3, 1.0, 0.8, 0.7, 0.9, 1.5, 0.0, -0.25)


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    yield e
    e.close()


def lowcov_stats(engine, report, oracle_stage2, check_table=False):
    pathcheck.check_stage2(engine, report("lowcov"), oracle_stage2("lowcov", max_distance=2), check_table=check_table)
    return engine.stats()


@pytest.fixture(scope="module")
def default_stats(engine, report, oracle_stage2):
    """Stats of the fixture with every pair in the exact table (no sketch) of 2048 slots: one pass per first k-mer."""
    with engine.knobs(dist_slots=2048, dist_block=128, dist_sketch=0):
        return lowcov_stats(engine, report, oracle_stage2)


@pytest.fixture(scope="module")
def small_stats(engine, report, oracle_stage2):
    """... and in tables of 256 slots: split passes."""
    with engine.knobs(dist_slots=256, dist_block=128, dist_sketch=0):
        return lowcov_stats(engine, report, oracle_stage2)


@pytest.mark.parametrize("int_thr", [1, 0])
@pytest.mark.parametrize("hot_entries", [32768, 0])
def test_dominance_ties_and_near_misses(engine, int_thr, hot_entries):
    """cnt / total >= thr exactly as the reference evaluates it (true division of two ints, a double compared with >=): a pair at
    exactly the threshold is an edge, one count short is not, at 0.5 / 0.6 / 0.75 / 0.3 / 1.0 / 0.8 (the integer test 5 cnt >= 4 total
    with dist_int_thr 1, the double division with 0) / 0.7 / 0.9 (these two fall below their threshold when divided in single
    precision); above 1 nothing is selected, at or below 0 every count >= min_cov is — with the filter's hot list and by its scan."""
    with engine.knobs(dist_int_thr=int_thr, dist_hot_entries=hot_entries):
        for thr in THRESHOLDS:
            pathcheck.check_tie_clouds(engine, thr)
        pathcheck.check_tie_clouds(engine, 0.8, copies=3)


@pytest.mark.parametrize("thr", [0.5, 0.3, 1.0])
def test_stage2_at_other_thresholds(engine, report, oracle_stage2, thr):
    """A1..A6 of the fixture at thresholds other than the default: the double division of the filter on real clouds."""
    with engine.knobs(dist_slots=2048, dist_block=128):
        pathcheck.check_stage2(engine, report("lowcov"), oracle_stage2("lowcov", max_distance=2), check_table=False, rel_threshold=thr)


def test_dist_int_thr_off(engine, report, oracle_stage2):
    """dist_int_thr 0: the default threshold 0.8 through the double division too (no trace in the stats: the edges are the check)."""
    with engine.knobs(dist_int_thr=0):
        lowcov_stats(engine, report, oracle_stage2)
        for thr in (0.8, 0.6):
            pathcheck.check_tie_clouds(engine, thr)


@pytest.mark.parametrize("hot_entries", [-1, 0, 1])
def test_dist_hot_entries(engine, report, oracle_stage2, hot_entries):
    """First k-mers with more partner entries than dist_hot_entries keep no hot list: the filter scans the table from the cursor the
    pass's set-up left (round 6; no trace in the stats).  -1 keeps the list always, 0 never, 1 for nearly no first k-mer."""
    with engine.knobs(dist_hot_entries=hot_entries, dist_slots=2048, dist_block=128):
        lowcov_stats(engine, report, oracle_stage2)
        pathcheck.check_tie_clouds(engine, 0.8)
        pathcheck.check_tie_clouds(engine, 0.5)
        with engine.knobs(dist_slots=4096):
            pathcheck.check_synthetic_clouds(engine, rel_threshold=0.05)


@pytest.mark.parametrize("fill", [10, 90])
def test_dist_fill_pct(engine, report, oracle_stage2, default_stats, small_stats, fill):
    """A (b, d) table pass is split once more than fill % of its slots are in use.  10 % of 2048 slots: more passes than at the
    default's 70 %, and split first k-mers where 70 % splits none.  90 % of 256 slots: the limit sits right under the physical size
    (a table this small keeps no slack for the drains' lag) — fewer passes than 70 %, and still split ones."""
    slots = 2048 if fill == 10 else 256
    with engine.knobs(dist_fill_pct=fill, dist_slots=slots, dist_block=128, dist_sketch=0):
        st = lowcov_stats(engine, report, oracle_stage2)
        pathcheck.check_tie_clouds(engine, 0.8)
    assert st["n_spilled"] > 0
    if fill == 10:
        assert default_stats["n_spilled"] == 0 and st["n_dist_passes"] > default_stats["n_dist_passes"], (st, default_stats)
    else:
        assert st["n_dist_passes"] < small_stats["n_dist_passes"], (st, small_stats)


@pytest.mark.parametrize("est", [5, 100])
def test_dist_est_pct(engine, report, oracle_stage2, small_stats, est):
    """The expected share of distinct (b, d) keys per pair emission sizes the first split of a first k-mer's pairs: at 5 % a first
    k-mer starts in fewer partitions and more of them fill up and split (n_spilled above the default 80 %'s); at 100 % it starts in
    more, fewer split, and there are more passes."""
    with engine.knobs(dist_est_pct=est, dist_slots=256, dist_block=128, dist_sketch=0):
        st = lowcov_stats(engine, report, oracle_stage2)
        pathcheck.check_tie_clouds(engine, 0.8)
    if est == 5:
        assert st["n_spilled"] > small_stats["n_spilled"], (st, small_stats)
    else:
        assert st["n_spilled"] < small_stats["n_spilled"] and st["n_dist_passes"] > small_stats["n_dist_passes"], (st, small_stats)


@pytest.mark.parametrize("shift", [0, 3])
def test_lut_shift(engine, report, oracle_stage2, default_stats, shift):
    """A3's k-mer lookup table with 1x and 8x the slots of its default (lut_shift -1 takes 4x for a set this small): the clouds, and
    the edges built on them, through build_clouds.  The table's size shows in the device memory held afterwards."""
    with engine.knobs(lut_shift=shift, dist_slots=2048, dist_block=128, dist_sketch=0):
        st = lowcov_stats(engine, report, oracle_stage2)
    if shift == 0:
        assert st["hbm_bytes_live"] < default_stats["hbm_bytes_live"]
    else:
        assert st["hbm_bytes_live"] > default_stats["hbm_bytes_live"]


@pytest.mark.parametrize("slots, tile", [(256, 64), (16384, 1)])
def test_count_table_knobs(engine, report, oracle_stage2, slots, tile):
    """count_slots (the per-read hash classes of the atomic counting path: fewest and most) and count_tile (reads per tile of its
    launch: one and the most) apply to count_mode 0 only; A1's whole table against the oracle.  (No trace in the stats: the table
    is the check.)"""
    with engine.knobs(count_mode=0, count_slots=slots, count_tile=tile):
        lowcov_stats(engine, report, oracle_stage2, check_table=True)


def test_synthetic_clouds_select_no_edge_at_the_default_threshold(engine):
    """(Why the tie clouds exist) the random clouds of check_synthetic_clouds spread every pair over many distances: at 0.8 they give
    no edge, so they check the emissions and the table's counts, not the filter's selection; at 0.05 they select some."""
    assert pathcheck.check_synthetic_clouds(engine).shape[0] == 0
    assert pathcheck.check_synthetic_clouds(engine, rel_threshold=0.05).shape[0] > 0

"""-m gpu: every knob of the distance stage's CPU matrix (test_emu_knobs.py) on a real MI355X, against the OpenMP oracle.

One read set of 1 000 reads of ~20 kb over units of 2 055 bp with substitutions, deletions, insertions and unit divergence
(~280 000 rare k-mers, ~57 000 pair emissions and ~750 selected edges per first k-mer: the hot list, the split table passes and
the sketch all run); its oracle record — A1..A3 and one partition a % 64 == 5 of the first k-mers — is computed once and every
knob setting must give the same counters, checksums, edges and unique k-mers (bigparity.check_record).  On top: the
dominance ties of pathcheck.tie_clouds on both paths of the default threshold, and the contig's overflow map of the placement
started tiny (place_cmap_bits) against the C placer.  No A/B build of cf_dist.hip runs here: those are test_emu_variants.py's."""
import numpy as np
import pytest

import bigparity
import pathcheck
from centroflye_amd import _host
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu
PART, N_PARTS = 5, 64
SETTINGS = [dict(dist_hot_entries=-1), dict(dist_hot_entries=0), dict(dist_hot_entries=1),
            dict(dist_fill_pct=10), dict(dist_fill_pct=90, dist_slots=256),
            dict(dist_est_pct=5), dict(dist_est_pct=100), dict(dist_int_thr=0),
            dict(lut_shift=0), dict(lut_shift=3),
            dict(count_mode=0, count_slots=256), dict(count_mode=0, count_slots=16384), dict(count_mode=0, count_tile=1), dict(count_mode=0, count_tile=64),
            dict(dist_sketch_bits=4), dict(dist_sketch_bits=8), dict(count_bits=4), dict(count_bits=16)]


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reads():
    pk = _host.synth(seed=11, n_reads=1000, unit_len=2055, var_len=8, mean_len=20000.0, max_len=200000, n_units=324,
                     p_sub=0.02, p_del=0.01, p_ins=0.01, unit_div=0.01)
    return pk, bigparity.oracle_record(pk, PART, N_PARTS)


@pytest.fixture(scope="module")
def default_run(engine, reads):
    pk, rec = reads
    r = bigparity.check_record(engine, pk, rec)
    assert r["identical"], r
    assert rec["partition"]["n_edges"] > 200 * rec["partition"]["n_first_kmers"], rec["partition"]      # (hundreds of edges per first k-mer)
    return r


@pytest.mark.parametrize("knobs", SETTINGS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_knob_setting_equals_the_oracle(engine, reads, default_run, knobs):
    pk, rec = reads
    with engine.knobs(**knobs):
        r = bigparity.check_record(engine, pk, rec)
    assert r["identical"], (knobs, r)
    if knobs.get("dist_fill_pct") == 10:      # (tables split at a tenth of their slots: more passes)
        assert r["got"]["n_dist_passes"] > default_run["got"]["n_dist_passes"], (r["got"], default_run["got"])


@pytest.mark.parametrize("int_thr", [1, 0])
def test_dominance_ties_and_near_misses(engine, int_thr):
    """pathcheck.tie_clouds at every threshold of test_emu_knobs.py, with the hot list and by the filter's scan."""
    for hot in (32768, 0):
        with engine.knobs(dist_int_thr=int_thr, dist_hot_entries=hot):
            for thr in (0.5, 0.6, 0.75, 0.3, 1.0, 0.8, 0.7, 0.9, 1.5, 0.0, -0.25):
                pathcheck.check_tie_clouds(engine, thr)
            pathcheck.check_tie_clouds(engine, 0.8, copies=3)


@pytest.mark.parametrize("bits", [3, 5])
def test_placement_with_a_tiny_contig_map_equals_the_c_placer(engine, bits):
    """place_cmap_bits: the contig's overflow map of cf_place2 starts with 2^bits slots and has to grow (round 5)."""
    from conftest import lines_from_placement
    from oracle import cport
    pk = _host.synth(seed=5, n_units=52, n_reads=130, var_len=8)
    up, us, ue, _ = pk.units(1)
    _, a = cport.stage2(pk.bases, pk.read_off, up, us, ue, 19, 3, 10, 32, 0, 2 ** 62, 1, 2, 4, 0.8, want_arrays=True)
    gk = a["rare"][a["unique"]]
    assert gk.size > 2000
    engine.load(pk, 1)
    engine.set_kmers(gk, 19); engine.build_clouds(); engine.filter_clouds(2)
    cp, ent = engine.clouds()
    cls = pk.classify(50000)
    rank = np.argsort(np.argsort(np.array(pk.ids, dtype=object), kind="stable"), kind="stable").astype(np.int32)
    want = lines_from_placement(pk.ids, *[x.tolist() for x in cport.place_reads(cls, rank, up, cp, ent, gk.size, 2, 2, 10, 3)])
    assert sum(1 for x in want if not x.endswith("None")) > 90
    with engine.knobs(place_cmap_bits=bits):
        got = lines_from_placement(pk.ids, *[x.tolist() for x in engine.place_reads(cls, rank, 2, 2, 10, 3)])
    assert got == want

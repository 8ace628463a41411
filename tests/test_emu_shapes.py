"""The shape cases of tests/shapecheck.py on the host-emulated build of the kernels: families 1 - 3 in full (cloud size
regimes of cf_cloud_kernel, read lengths / alignments / symbols in A1's first pass, few reads with repeats), the two small
cases and the first dense one of family 4.  The emulator runs threads as fibers: it checks the branches' logic, not their
wave-level behaviour — tests/test_gpu_shapes.py runs the same cases on an MI355X."""
import numpy as np
import pytest

import shapecheck
from centroflye_amd import _host
from centroflye_amd.engine import Engine


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = Engine(0, emu_lib)
    e.set_param("dist_slots", 2048)      # (a small distance kernel: the emulator's time per launch goes with its threads and LDS)
    e.set_param("dist_block", 128)
    yield e
    e.close()


def test_naive_reference_equals_the_oracle_on_tiny(report, oracle_stage2):
    """The plain restatement every case here is judged by, pinned first: table, rare set, clouds, edges and unique k-mers of
    the `tiny` fixture as oracle/recruit.py computes them."""
    records, alns, lens, res, p2 = oracle_stage2("tiny")
    pk = _host.parse_report(report("tiny"))
    up, us, ue, _ = pk.units(1)
    reads, units = shapecheck.from_arrays(pk.bases, pk.read_off, up, us, ue)
    cn = res["counters"]
    nv = shapecheck.naive_stage2(reads, units, p2["k"], p2["max_nonuniq"], cn["lo"], cn["hi"], min_d=p2["min_distance"],
                                 max_d=p2["max_distance"], min_cov=p2["min_coverage"], thr=0.8)
    ok = nv["multi"] <= p2["max_nonuniq"]
    assert (nv["n_bases"], nv["n_windows"], nv["n_read_kmers"], nv["n_distinct"]) == (cn["n_b"], cn["n_w"], cn["n_rk"], cn["n_distinct"])
    assert nv["n_plain"] == nv["n_windows"]
    assert np.array_equal(nv["keys"][ok], res["keys"]) and np.array_equal(nv["pres"][ok].astype(np.int64), res["pres"])
    assert np.array_equal(nv["set_codes"], res["rare"]) and res["rare"].size > 1000
    assert np.array_equal(nv["cloud_ptr"], res["cloud_ptr"]) and np.array_equal(nv["entries"], res["entries"])
    assert nv["E"] == cn["E"] and res["edges"].shape[0] > 1000
    assert np.array_equal(nv["edges"], res["edges"]) and np.array_equal(nv["unique"], res["unique"])


# ------------------------------------------------------------------ family 1: cloud size regimes
@pytest.mark.parametrize("n", shapecheck.CLOUD_SIZES)
def test_cloud_size_regimes(engine, n):
    shapecheck.check_shapes(engine, shapecheck.cloud_size_case(n))


def test_cloud_beyond_the_lds_set_is_refused_and_the_context_stays_usable(engine):
    """6145 distinct set k-mers in one unit: cf_build_clouds returns -34 (a host-side code, checked before any result is
    used); the same context then builds the 1536-entry case."""
    shapecheck.check_shapes(engine, shapecheck.cloud_size_case(6145))
    shapecheck.check_shapes(engine, shapecheck.cloud_size_case(1536))


def test_retry_repeats_units_that_had_fitted(engine):
    shapecheck.check_shapes(engine, shapecheck.cloud_mixed_case())


def test_cloud_staging_tile_borders(engine):
    shapecheck.check_shapes(engine, shapecheck.cloud_staging_case())


# ------------------------------------------------------------------ family 2: A1's first pass
@pytest.mark.parametrize("k", shapecheck.A1_KS)
def test_a1_lengths_alignments_and_symbols(engine, k):
    """Sort and reduce (count_mode 1; k = 30, 31 take the table path by themselves), then A3 and A4 on whole reads as units
    (and the distance stage on the first read set); the atomic table (count_mode 0) up to the rare set."""
    for e in range(4):
        for symbols in (0, 1):
            case = shapecheck.a1_case(k, e, symbols)
            shapecheck.check_shapes(engine, case, dist=(e == 0))
            with engine.knobs(count_mode=0):
                shapecheck.check_shapes(engine, case, upto="A2")


# ------------------------------------------------------------------ family 3: few reads, repeats
@pytest.mark.parametrize("k", [4, 11, 19, 25])
@pytest.mark.parametrize("R", [1, 2, 3, 5])
def test_few_reads_with_repeats(engine, R, k):
    """A1 -> A4 at max_nonuniq 0, 1, 2, the distance stage at 2 (the emulated launches are what costs here; the GPU suite runs
    it at all three); occurrence counts and top n on both A1 paths."""
    for max_nonuniq in (0, 1, 2):
        shapecheck.check_shapes(engine, shapecheck.repeats_case(R, k, max_nonuniq), dist=(max_nonuniq == 2))
    reads = shapecheck.repeats_case(R, k, 0)["reads"]
    shapecheck.check_occurrences(engine, reads, k, ns="few")
    with engine.knobs(count_mode=0):
        shapecheck.check_occurrences(engine, reads, k, ns="one")


# ------------------------------------------------------------------ family 4: dense clouds through the distance stage
@pytest.mark.parametrize("name", shapecheck.DENSE_SMALL + ("dense_2x5",))
def test_dense_clouds(engine, name):
    shapecheck.check_dense(engine, name)

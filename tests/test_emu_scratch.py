"""tests/scratchcheck.py on the host emulator, and the one check that only the emulator can make: every exit that a failed
allocation takes.  cfemu_fail_allocs_from(n) (tests/emu/cfemu_runtime.cpp) makes the n-th hipMalloc after the call and every later
one fail; for n = 1, 2, 3, ... a fresh context (an empty pool: the count is deterministic) runs the sequence up to the call that
fails, then runs it whole."""
import re

import pytest

import scratchcheck
from centroflye_amd.engine import DeviceError, Engine

STAGES = ("cf_count_kmers", "cf_build_clouds", "cf_dist_edges", "cf_contig_build", "cf_map_reads", "cf_score_reads", "cf_tandem_scan")


def _engine(lib):
    e = Engine(0, lib)
    e.set_param("dist_slots", 2048)      # (a small distance kernel: the emulator's time per launch goes with its threads and LDS)
    e.set_param("dist_block", 128)
    return e


@pytest.fixture(scope="module")
def engine(emu_lib):
    e = _engine(emu_lib)
    yield e
    e.close()


def test_every_call_gives_back_what_it_took(engine, report):
    scratchcheck.check_balanced(engine, report)


def test_refusals_behind_an_allocation_give_it_back(engine, report):
    scratchcheck.check_refusals(engine, report)


def test_every_exit_of_a_failed_allocation(emu_lib, report):
    steps = scratchcheck.SMALL_STEPS
    with _engine(emu_lib) as clean:
        scratchcheck.sequence(clean, report, steps)
        want_live = clean.stats()["hbm_bytes_live"]
    hit, bad, n = {}, [], 0
    try:
        while True:
            n += 1
            with _engine(emu_lib) as e:
                emu_lib.cfemu_fail_allocs_from(n)
                try:
                    scratchcheck.sequence(e, report, steps)
                    failed = None
                except DeviceError as err:
                    failed = str(err)
                emu_lib.cfemu_fail_allocs_from(0)
                if failed is None:
                    break
                m = re.match(r"(\w+) failed \((-?\d+)\): hipMalloc of \d+ bytes for (.*?): ", failed)
                assert m and m.group(2) == "-12", f"allocation {n}: {failed}"
                hit.setdefault(m.group(1), set()).add(m.group(3))
                scratchcheck.sequence(e, report, steps)      # (every result against its reference)
                live = e.stats()["hbm_bytes_live"]
                if live != want_live:
                    bad.append(f"allocation {n} failed for {m.group(3)} in {m.group(1)}: {live} bytes live afterwards")
    finally:
        emu_lib.cfemu_fail_allocs_from(0)
    assert not bad, f"{want_live} bytes are live on a context that saw no failure; " + "; ".join(bad)
    missing = [call for call in STAGES if call not in hit]
    assert not missing, f"no allocation failed inside {missing}: {sorted(hit.items())}"

"""The diagnostic builds of the distance and counting kernels (compile-time switches of cf_dist.hip and cf_count2.hip, built for the
GPU by tools/build_variant.sh) compute what the default build computes — checked on the host emulator, each build in a process of
its own (a build that writes out of bounds fails its test instead of the suite).  Every build runs the dominance-tie clouds, the
random clouds of pathcheck.check_synthetic_clouds (a multi-chunk posting list, at a threshold that selects edges) and A1..A6 of the
lowcov fixture, under knobs that force the rare paths (no hot list, no sketch, a small table) and under the defaults.

Result-preserving builds, by their comments in cf_dist.hip / cf_count2.hip:
  CF_DIST_STAMPS, CF_C2_STAMPS   per-phase clock sums of the distance / counting kernels (the host's clock is a counter)
  CF_DIST_DIAG_NOHOT        no first k-mer keeps the hot list (the filter scans; it read an empty list and selected nothing before)
  CF_DIST_DIAG_COUNT        counters of the parked inserts and drains, printed per launch
Not here:
  CF_NO_BUFFER_LOAD         the emulator's own build defines it: every emulator test runs it
  CF_PL2_STAMPS / _STAMPS2  placement, not the distance stage (test_emu_kernels.py covers its kernels)
(The A/B switches of the distance kernel's insert path, rounds 2 to 6, are retired: DESIGN.md, "Retired compile-time switches".)"""
import os
import pickle
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {
    "dist_stamps": ["-DCF_DIST_STAMPS"],
    "c2_stamps": ["-DCF_C2_STAMPS"],
    "diag_nohot": ["-DCF_DIST_DIAG_NOHOT"],
    "diag_count": ["-DCF_DIST_DIAG_COUNT"],
}
# (knob settings, run the random clouds too)
SETTINGS = [(dict(dist_hot_entries=0, dist_sketch=0, dist_slots=1024), True),
            (dict(dist_slots=2048, dist_block=128), False)]
RUN = r"""
import pickle, sys
root, lib_path, report_path, oracle_path, settings = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], eval(sys.argv[5])
sys.path[:0] = [root, root + "/tests"]
import pathcheck
from centroflye_amd import _lib
from centroflye_amd.engine import Engine
tup = pickle.load(open(oracle_path, "rb"))
e = Engine(0, _lib.load(lib_path))
for knobs, clouds in settings:
    with e.knobs(**knobs):
        for thr in (0.8, 0.6, 0.0):
            pathcheck.check_tie_clouds(e, thr)
        if clouds:
            assert pathcheck.check_synthetic_clouds(e, rel_threshold=0.05).shape[0] > 0
        pathcheck.check_stage2(e, report_path, tup, check_table=False)
print("VARIANT-OK")
"""


@pytest.fixture(scope="module")
def results(emu_lib, report, oracle_stage2, tmp_path_factory):
    oracle_path = str(tmp_path_factory.mktemp("variants") / "lowcov_d2.pkl")
    with open(oracle_path, "wb") as f:
        pickle.dump(oracle_stage2("lowcov", max_distance=2), f)
    report_path = report("lowcov")

    def one(name):
        b = subprocess.run(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh"), name] + VARIANTS[name], capture_output=True, text=True, timeout=900)
        if b.returncode:
            return "build failed: " + b.stderr[-3000:]
        lib = os.path.join(ROOT, "tests", "emu", f"libcfhip_emu_{name}.so")
        r = subprocess.run([sys.executable, "-c", RUN, ROOT, lib, report_path, oracle_path, repr(SETTINGS)],
                           capture_output=True, text=True, timeout=900)
        return "ok" if r.returncode == 0 and "VARIANT-OK" in r.stdout else f"exit {r.returncode}: " + r.stdout[-2000:] + r.stderr[-3000:]

    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        return dict(zip(VARIANTS, pool.map(one, VARIANTS)))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_build_computes_what_the_default_computes(results, name):
    assert results[name] == "ok", f"{name} {VARIANTS[name]}: {results[name]}"

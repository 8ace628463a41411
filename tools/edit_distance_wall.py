#!/usr/bin/env python3
"""Device time of the polisher's comparisons (cf_hpc + cf_edit_distances) against the reference's edlib in mode NW on
one host core of the same machine, in the same run (edlibAlign of oracle/_ref/librr_ref.so, the reference's vendored edlib).

  (a) cenX shape: the six comparisons of a --num-iters 4 run, 1 500 positions x 2 055 bases, successive iterations differing by
      1e-3 substitutions and indels per base;
  (b) the same at 15 000 positions (the bench's size);
  (c) give-up time: two unrelated strings of 1 Mb at --max-edit-distance limits from the default downwards.

Device ms are HIP-event times of cf_edit_distances (copies of the offsets included; the sequences are resident after cf_hpc),
median of --reps after --warmup; cf_hpc is timed on the host around the call.  edlib is run once per comparison (it takes
seconds to minutes); --edlib-pairs-b limits it in case (b) to the last N of the six comparisons, each compared on its own.

    python tools/edit_distance_wall.py --out profiles/r12_edit_distance.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centroflye_amd.engine import Engine  # noqa: E402
from centroflye_amd.eltr_polisher import DEFAULT_MAX_EDIT_DISTANCE  # noqa: E402


class _Config(C.Structure):
    _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int), ("additionalEqualities", C.c_void_p), ("additionalEqualitiesLength", C.c_int)]


class _Result(C.Structure):
    _fields_ = [("status", C.c_int), ("editDistance", C.c_int), ("endLocations", C.POINTER(C.c_int)), ("startLocations", C.POINTER(C.c_int)),
                ("numLocations", C.c_int), ("alignment", C.c_void_p), ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]


def edlib_nw():
    path = os.path.join(ROOT, "oracle", "_ref", "librr_ref.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.edlibAlign.restype = _Result
    lib.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _Config]
    lib.edlibFreeAlignResult.argtypes = [_Result]

    def nw(a, b):
        t = time.perf_counter()
        r = lib.edlibAlign(a, len(a), b, len(b), _Config(-1, 0, 0, None, 0))
        ms = (time.perf_counter() - t) * 1e3
        d = r.editDistance
        lib.edlibFreeAlignResult(r)
        return d, ms
    return nw


def mutate(rng, s, rate):
    """rate * len(s) edits: a third each substitutions, insertions, deletions (numpy, whole array at a time)."""
    n = max(1, int(s.size * rate / 3))
    s = s.copy()
    p = rng.integers(0, s.size, n)
    s[p] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), s[p]) + rng.integers(1, 4, n)) % 4]
    s = np.delete(s, rng.integers(0, s.size, n))
    return np.insert(s, rng.integers(0, s.size, n), np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def polishing_run(rng, positions, unit_len=2055, iters=4, rate=1e-3):
    unit = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, unit_len)]
    seq = np.tile(unit, positions)
    p = rng.integers(0, seq.size, seq.size // 50)       # 2 % divergence between the units of the array
    seq[p] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, p.size)]
    seqs = [seq]
    for _ in range(iters - 1):
        seqs.append(mutate(rng, seqs[-1], rate))
    return seqs


def time_case(e, seqs, limit, reps, warmup, edlib, edlib_pairs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([s.size for s in seqs], out=off[1:])
    data = np.concatenate(seqs)
    hpc_ms = []
    for _ in range(1 + min(reps, 2)):
        t = time.perf_counter()
        hpc, hpc_off = e.hpc(data, off)
        hpc_ms.append((time.perf_counter() - t) * 1e3)
    # the pair list of eltr_polisher.assemble: plain (i, i + 1), two joining pairs with an empty string, compressed (i, i + 1)
    n = len(seqs)
    h = off[-1] + hpc_off
    a_off = np.concatenate([off, off[-1:], h[1:n]])
    b_off = np.concatenate([off[1:], off[-1:], h[1:]])
    ms = []
    for i in range(warmup + reps):
        d, t = e.edit_distances(None, a_off, b_off, limit)
        if i >= warmup:
            ms.append(t)
    pairs = [("plain", i, seqs[i].tobytes(), seqs[i + 1].tobytes(), int(d[i])) for i in range(n - 1)]
    pairs += [("hpc", i, hpc[hpc_off[i]:hpc_off[i + 1]].tobytes(), hpc[hpc_off[i + 1]:hpc_off[i + 2]].tobytes(), int(d[n + 1 + i])) for i in range(n - 1)]
    rec = dict(bases=[int(s.size) for s in seqs], hpc_bases=np.diff(hpc_off).tolist(), limit=int(limit),
               distances={f"{w}_{i + 1}v{i + 2}": dd for w, i, _, _, dd in pairs},
               edit_ms_median=statistics.median(ms), edit_ms_all=[round(x, 3) for x in ms], hpc_wall_ms=[round(x, 3) for x in hpc_ms])
    if edlib is not None and edlib_pairs > 0:
        rec["edlib_one_core_ms"] = {}
        # per comparison: the same pair alone on the device, and edlib on one core
        for w, i, a, b, dd in pairs[-edlib_pairs:] if edlib_pairs < len(pairs) else pairs:
            one = [e.edit_distances(a + b, [0, len(a)], [len(a), len(a) + len(b)], limit)[1] for _ in range(3)]
            want, ems = edlib(a, b)
            assert want == dd or dd == -1, (w, i, want, dd)
            rec["edlib_one_core_ms"][f"{w}_{i + 1}v{i + 2}"] = dict(edlib_ms=round(ems, 1), device_ms_alone=round(min(one), 3), distance=want)
        rec["edlib_ms_sum"] = round(sum(v["edlib_ms"] for v in rec["edlib_one_core_ms"].values()), 1)
        rec["not_slower_than_edlib"] = rec["edit_ms_median"] <= rec["edlib_ms_sum"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_edit_distance.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--edlib-pairs-b", type=int, default=2, help="comparisons of case (b) that edlib is run on (the last ones: the smallest distances)")
    ap.add_argument("--limits-c", default="65536,32768,16384,8192", help="limits of case (c): from the issue's first default downwards")
    args = ap.parse_args()
    rng = np.random.default_rng(12)
    edlib = edlib_nw()
    out = dict(tool="tools/edit_distance_wall.py", reps=args.reps, warmup=args.warmup, default_max_edit_distance=DEFAULT_MAX_EDIT_DISTANCE,
               edlib="oracle/_ref/librr_ref.so, mode NW, k = -1, one core" if edlib else None)
    with Engine(0) as e:
        out["device"] = e.device_info()
        out["kernel"] = e.edit_info()
        if "a" in args.cases:
            out["a_cenx_1500_positions"] = time_case(e, polishing_run(rng, 1500), DEFAULT_MAX_EDIT_DISTANCE, args.reps, args.warmup, edlib, 6)
            print("a", json.dumps(out["a_cenx_1500_positions"])[:600], flush=True)
        if "b" in args.cases:
            out["b_15000_positions"] = time_case(e, polishing_run(rng, 15000), DEFAULT_MAX_EDIT_DISTANCE, args.reps, args.warmup, edlib, args.edlib_pairs_b)
            print("b", json.dumps(out["b_15000_positions"])[:600], flush=True)
        if "c" in args.cases:
            a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1000000)].tobytes()
            b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1000000)].tobytes()
            out["c_give_up_1mb_unrelated"] = {}
            for limit in [int(x) for x in args.limits_c.split(",")]:
                ms = []
                for i in range(1 + 3):
                    d, t = e.edit_distances(a + b, [0, len(a)], [len(a), 2 * len(a)], limit)
                    assert int(d[0]) == -1
                    if i >= 1:
                        ms.append(t)
                out["c_give_up_1mb_unrelated"][str(limit)] = dict(ms_median=statistics.median(ms), ms_all=[round(x, 2) for x in ms])
                print("c", limit, ms, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

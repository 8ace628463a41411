#!/usr/bin/env python3
"""Device time of the exact mono-k-mer counts (cf_monokmers_run) and of the iterative graph on them, on D6Z1-shaped
monostrings: 50 000 strings of about 120 letters (6e6 letters) that read the 18-letter HOR cyclically from a random phase, with
the generator's error rates turned into gaps and substitutions.

  --device     (needs the GPU) median of 3 runs after 1 warm-up, by HIP events (cf_monokmers_info): one call at k = 3, 100 and 400
               with the sorts' share, the sorts and 8-bit passes a call runs; then iterative_graph for k = --min-k .. --max-k: wall
               time, the device milliseconds summed over its calls, and the rest (Python: strings, dicts, the graph).
  --reference DIR   (build container only; one host core) the reference's own get_frequent_kmers at k = 3 and 100 and iterative_graph
               on --ref-strings strings, a size it finishes in minutes; the tool also prints windows x k of both sizes so that the
               figure can be SCALED to the device's input — a scaled figure, not a measured one.
usage: python tools/monokmers_wall.py --device --out profiles/r29_monokmers.json
       python tools/monokmers_wall.py --reference /path/to/reference --out profiles/r29_monokmers_reference.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOR = np.frombuffer(b"ABCDEFGHIJKLMNOPQR", np.uint8)
SUB, GAPS = 0.02, 0.035      # substitutions; insertions + deletions of the generator, seen as unreliable instances


def strings(n, seed=29, mean_len=120):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = int(rng.integers(mean_len - 40, mean_len + 41))
        x = HOR[(int(rng.integers(0, 18)) + np.arange(m)) % 18].copy()
        sub = rng.random(m) < SUB
        x[sub] = rng.integers(65, 83, int(sub.sum()))
        x[rng.random(m) < GAPS] = ord("?")
        out.append(x.tobytes())
    return out


def windows_times_k(strs, ks):
    return {k: sum(max(len(s) - k + 1, 0) for s in strs) * k for k in ks}


def device(args):
    from centroflye_amd import debruijn_graph, session
    strs = strings(args.strings)
    e = session.engine()
    res = {"device": e.device_info()["name"], "n_strings": len(strs), "n_letters": sum(map(len, strs)), "calls": [],
           "windows_times_k": windows_times_k(strs, (3, 100, 400))}
    flat = np.frombuffer(b"".join(strs), np.uint8)
    off = np.zeros(len(strs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strs])
    for k, mm in ((3, 5000), (100, 5), (400, 5)):
        runs = []
        for it in range(4):
            t0 = time.perf_counter()
            e.monokmers((flat, off), k, mm, True)
            wall = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append(dict(e.monokmers_info()["phase_ms"], wall_ms=wall))
        info = e.monokmers_info()
        med = {key: statistics.median(r[key] for r in runs) for key in runs[0]}
        res["calls"].append({"k": k, "min_mult": mm, "median_ms": med, "runs": runs, "sort_share": med["sorts"] / med["total"] if med["total"] else None,
                             **{key: info[key] for key in ("n_windows", "n_distinct", "n_kmers", "n_occ", "n_rounds", "n_sorts", "n_sort_passes")}})
        print(json.dumps(res["calls"][-1]), flush=True)
    # the iterative graph: device milliseconds summed over the calls it makes
    dev_ms, n_calls = [0.0], [0]
    inner = e.monokmers

    def counted(*a, **kw):
        out = inner(*a, **kw)
        dev_ms[0] += e.monokmers_info()["phase_ms"]["total"]
        n_calls[0] += 1
        return out
    e.monokmers = counted
    mono = {"s%05d" % x: types.SimpleNamespace(string=list(s.decode())) for x, s in enumerate(strs)}
    for ms in mono.values():
        ms.tostring = lambda ms=ms: "".join(ms.string)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        contigs, _, frequent, _ = debruijn_graph.iterative_graph(mono, min_k=args.min_k, max_k=args.max_k, outdir=os.path.join(tmp, "idb"), min_mult=5, verbose=False)
        wall = time.perf_counter() - t0
    res["iterative_graph"] = {"min_k": args.min_k, "max_k": args.max_k, "wall_s": wall, "device_s": dev_ms[0] / 1e3, "python_s": wall - dev_ms[0] / 1e3,
                              "device_calls": n_calls[0], "device_ms_per_k": dev_ms[0] / (args.max_k - args.min_k + 1),
                              "frequent_kmers_at_min_k": len(frequent[args.min_k]), "contigs_at_min_k": len(contigs[args.min_k])}
    print(json.dumps(res["iterative_graph"]), flush=True)
    return res


def reference(args):
    sys.dont_write_bytecode = True
    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, bio.SeqIO
    import networkx
    networkx.drawing.nx_pydot.write_dot = lambda graph, path: None
    sys.path.insert(0, os.path.join(args.reference, "scripts"))
    import debruijn_graph as RG
    strs = strings(args.ref_strings)
    plain = {"s%05d" % x: s.decode() for x, s in enumerate(strs)}
    res = {"host": "one core", "n_strings": len(strs), "n_letters": sum(map(len, strs)), "calls": [],
           "windows_times_k": windows_times_k(strs, (3, 100, 400)), "full_size_windows_times_k": windows_times_k(strings(args.strings), (3, 100, 400))}
    for k, mm in ((3, 500), (100, 5)):
        t0 = time.perf_counter()
        frequent, _ = RG.get_frequent_kmers(plain, k=k, min_mult=mm)
        res["calls"].append({"k": k, "seconds": time.perf_counter() - t0, "n_kmers": len(frequent)})
        print(json.dumps(res["calls"][-1]), flush=True)
    mono = {r: types.SimpleNamespace(string=list(s)) for r, s in plain.items()}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        RG.iterative_graph(mono, min_k=args.min_k, max_k=args.max_k, outdir=os.path.join(tmp, "idb"), min_mult=5, verbose=False)
        res["iterative_graph"] = {"min_k": args.min_k, "max_k": args.max_k, "seconds": time.perf_counter() - t0}
    print(json.dumps(res["iterative_graph"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--reference")
    ap.add_argument("--strings", type=int, default=50000)
    ap.add_argument("--ref-strings", type=int, default=5000)
    ap.add_argument("--min-k", type=int, default=100)
    ap.add_argument("--max-k", type=int, default=400)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"tool": "tools/monokmers_wall.py", "error_rates": {"sub": SUB, "gaps": GAPS}}
    if args.device:
        res["device_run"] = device(args)
    if args.reference:
        res["reference_run"] = reference(args)
    if args.out:
        with open(args.out + ".tmp", "w") as f:
            json.dump(res, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of mapping monoreads to the graph's edges (cf_monomap_run) and wall time of DeBruijnGraph.map_reads on it.
The edges are a planted array of the 18-letter HOR in which every unit carries another monomer at one place (so that long windows
are unique), cut into --edges edges; the reads are pieces of the array with substitutions and gaps.

  --device     (needs the GPU) median of 3 runs after 1 warm-up, phase times by HIP events (cf_monomap_info) and the wall time of one
               map_reads call: the shape of DESIGN §29 (50 000 reads of about 120 letters, k = 100) and long reads (--long-reads reads
               of --long-len letters, k = 100 and 400).
  --reference DIR   (build container only; one host core) the reference's own map_reads — index_edges included, which it runs first —
               on the long reads scaled down to --ref-reads reads; the tool prints the read letters of both sizes so that the figure can
               be SCALED (index_edges does not grow with the reads: its seconds are given apart) — a scaled figure, not a measured one.
usage: python tools/monomap_wall.py --device --out profiles/r33_monomap.json
       python tools/monomap_wall.py --reference /path/to/reference --out profiles/r33_monomap_reference.json"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOR = np.frombuffer(b"ABCDEFGHIJKLMNOPQR", np.uint8)
SUB, GAPS = 0.002, 0.002      # what error correction leaves: a few wrong monomers and gaps


def array_and_edges(n_units, n_edges, seed=33):
    rng = np.random.default_rng(seed)
    array = np.tile(HOR, n_units)
    array[7::18] = HOR[(7 + rng.integers(1, 18, n_units)) % 18]      # another monomer at place 7 of every unit
    cuts = np.linspace(0, len(array), n_edges + 1).astype(int)
    return array, [array[a:b].tobytes() for a, b in zip(cuts[:-1], cuts[1:])]


def reads_of(array, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = int(rng.integers(lo, hi + 1))
        a = int(rng.integers(0, len(array) - m + 1))
        x = array[a:a + m].copy()
        sub = rng.random(m) < SUB
        x[sub] = rng.integers(65, 83, int(sub.sum()))
        x[rng.random(m) < GAPS] = ord("?")
        out.append(x.tobytes())
    return out


def shapes(args):
    array, edges = array_and_edges(args.units, args.edges)
    return edges, [("the shape of DESIGN 29: 50 000 reads of about 120 letters", reads_of(array, args.short_reads, 80, 160, 1), (100,)),
                   ("long reads", reads_of(array, args.long_reads, args.long_len * 3 // 4, args.long_len * 5 // 4, 2), (100, 400))], array


def hand_graph(G, edges, k):
    """a graph whose edges are the given strings, one after the other"""
    db = G.DeBruijnGraph(k=k)
    for x, s in enumerate(edges):
        db.graph.add_edge(x, x + 1, edge_kmer=s.decode(), coverages=[10] * max(len(s) - k + 1, 1), length=max(len(s) - k + 1, 1), color="blue")
    return db


def device(args):
    from centroflye_amd import debruijn_graph, session
    edges, sets, _ = shapes(args)
    e = session.engine()
    res = {"device": e.device_info()["name"], "n_edges": len(edges), "edge_letters": sum(map(len, edges)), "calls": []}
    uv = [(x, x + 1) for x in range(len(edges))]
    for name, reads, ks in sets:
        for k in ks:
            runs = []
            for it in range(4):
                e.monomap(edges, uv, reads, k)
                if it:
                    runs.append(dict(e.monomap_info()["phase_ms"]))
            info = e.monomap_info()
            db = hand_graph(debruijn_graph, edges, k)
            mono = {"s%06d" % x: s.decode() for x, s in enumerate(reads)}
            t0 = time.perf_counter()
            mapping = db.map_reads(mono, verbose=False, engine=e)
            wall = time.perf_counter() - t0
            med = {key: statistics.median(r[key] for r in runs) for key in runs[0]}
            res["calls"].append({"shape": name, "k": k, "n_reads": len(reads), "read_letters": sum(map(len, reads)), "median_ms": med, "runs": runs,
                                 "sort_share": med["sorts"] / med["total"] if med["total"] else None, "map_reads_wall_s": wall,
                                 "mapped_reads": sum(m is not None for m in mapping.values()),
                                 **{key: info[key] for key in ("n_edge_windows", "n_indexed", "n_hits", "n_path", "n_rounds", "n_sorts")}})
            print(json.dumps(res["calls"][-1]), flush=True)
    return res


def reference(args):
    sys.dont_write_bytecode = True
    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, bio.SeqIO
    import networkx  # noqa: F401
    sys.path.insert(0, os.path.join(args.reference, "scripts"))
    import debruijn_graph as RG
    edges, sets, array = shapes(args)
    full = sets[1][1]
    reads = reads_of(array, args.ref_reads, args.long_len * 3 // 4, args.long_len * 5 // 4, 2)
    res = {"host": "one core", "n_edges": len(edges), "edge_letters": sum(map(len, edges)), "n_reads": len(reads), "read_letters": sum(map(len, reads)),
           "full_size_reads": len(full), "full_size_read_letters": sum(map(len, full)), "calls": []}
    mono = {"s%06d" % x: types.SimpleNamespace(string=list(s.decode())) for x, s in enumerate(reads)}
    for k in (100, 400):
        db = hand_graph(RG, edges, k)
        t0 = time.perf_counter()
        db.index_edges()
        t1 = time.perf_counter()
        mapping = db.map_reads(mono, verbose=False)
        t2 = time.perf_counter()
        res["calls"].append({"k": k, "index_edges_s": t1 - t0, "map_reads_behind_the_index_s": t2 - t1, "mapped_reads": sum(m is not None for m in mapping.values())})
        print(json.dumps(res["calls"][-1]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--reference")
    ap.add_argument("--units", type=int, default=600, help="HOR units of the planted array (18 letters each)")
    ap.add_argument("--edges", type=int, default=12)
    ap.add_argument("--short-reads", type=int, default=50000)
    ap.add_argument("--long-reads", type=int, default=2000)
    ap.add_argument("--long-len", type=int, default=5000)
    ap.add_argument("--ref-reads", type=int, default=100)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"tool": "tools/monomap_wall.py", "error_rates": {"sub": SUB, "gaps": GAPS}}
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

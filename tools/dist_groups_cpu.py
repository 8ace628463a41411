#!/usr/bin/env python3
"""How much of the distance stage's sweep would GROUPS of first k-mers save?  CPU only, no GPU.

cnt(a, b, d) = #{u in L(a) : b in cloud(u + d)}, L(a) the posting list of the first k-mer a.  First k-mers with the same first posting unit come
from one place of the array: their lists are subsets of one column of read units.  DESIGN.md 24 sweeps k-mers with EQUAL lists once (classes).
A group sweeps the UNION of its members' lists once and keeps, per (b, d), a bit mask of the union's postings that contributed; member j with
list mask M_j then has cnt = popcount(mask & M_j).  This tool counts, on generator reads, what that would sweep:

  * first k-mers, classes (distinct posting lists), list lengths;
  * per cap on the union's size: groups, classes and k-mers per group, the partner entries of the unions against the partner entries swept with
    classes (the sweep, push, insert, clear and per-pass fixed cost scale with it), and sum over groups of members x union entries against the
    entries of the classes (a proxy for the per-member filter, which reads the union's table once per member).

Partner entries of a posting at unit u are the kernel's item ranges: the clouds of the units u + min_d .. min(read end, u + max_d).
Groups are formed greedily: the k-mers of one first unit in some order, a group closed when the union would pass the cap or the members reach
255 (DIST_CLASS_CAP); a list longer than the cap is a group of its own.  The order decides how small the unions stay (--order):
  list    ascending order of the lists themselves (the measurement the idea started from)
  second  by the second posting unit, then the list's length — close to what the library's order key [first unit | low bits of the second unit | rank] gives
  hash    by a hash of the list, the order key of the classes: neighbours are unrelated and the unions fill up early

  python tools/dist_groups_cpu.py --reads 3000 --reads 6000            # the bench's generator (seed 2, var_len 8, n_units = 0.3 x reads)
  python tools/dist_groups_cpu.py --cenx --var-len 8 --var-len 1       # bench.py's CENX shape
  ... --json out.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (K, PARAMS, CENX, synth_kwargs: the workloads are the benchmark's)

CLASS_CAP = 255


def clouds_of(synth_kw):
    from centroflye_amd import _host
    from oracle import cport
    pk = _host.synth(**synth_kw)
    up, us, ue, _ = pk.units(1)
    P = bench.PARAMS
    with cport.Stage2State(pk.bases, pk.read_off, up, us, ue, bench.K, P["max_nonuniq"], P["lo"], P["hi"], threads=0) as st:
        arr = st.arrays()
    return np.asarray(up, np.int64).copy(), arr["cloud_ptr"], arr["entries"]


def partner_entries(unit_ptr, cloud_ptr, min_d, max_d):
    """per unit: the cloud entries of its partner units (cf_unit_rend_kernel's urange.len)"""
    n_units = cloud_ptr.size - 1
    rend = np.repeat(unit_ptr[1:], np.diff(unit_ptr))
    assert rend.size == n_units
    u = np.arange(n_units, dtype=np.int64)
    jlo, jhi = u + min_d, np.minimum(rend - 1, u + max_d)
    ok = jhi >= jlo
    return np.where(ok, cloud_ptr[np.where(ok, jhi, 0) + 1] - cloud_ptr[np.where(ok, jlo, 0)], 0)


def posting_lists(cloud_ptr, entries):
    """the posting list (ascending units) of every k-mer that occurs, as tuples"""
    unit = np.repeat(np.arange(cloud_ptr.size - 1, dtype=np.int64), np.diff(cloud_ptr))
    o = np.argsort(entries, kind="stable")
    r, u = entries[o], unit[o]
    cut = [0] + (np.flatnonzero(np.diff(r)) + 1).tolist() + [int(r.size)]
    ul = u.tolist()
    return [tuple(ul[i:j]) for i, j in zip(cut[:-1], cut[1:]) if j > i]


def measure(unit_ptr, cloud_ptr, entries, caps, min_d, max_d, order="list"):
    plen = partner_entries(unit_ptr, cloud_ptr, min_d, max_d).tolist()
    lists = posting_lists(cloud_ptr, entries)
    lens = np.array([len(x) for x in lists])
    ent = lambda L: sum(plen[x] for x in L)      # noqa: E731
    # the order inside a run of one first unit: by the lists themselves, by (second unit, list length), or by a hash of the list (the
    # order keys of DESIGN.md 24 put a hash below the first unit)
    key_of = (lambda L: (L[1] if len(L) > 1 else -1, len(L), hash(L))) if order == "second" else (lambda L: hash(L))
    by_first = {}
    for L in lists:
        by_first.setdefault(L[0], {}).setdefault(L, 0)
        by_first[L[0]][L] += 1
    n_classes = sum(len(v) for v in by_first.values())
    e_kmers = sum(ent(L) * n for v in by_first.values() for L, n in v.items())
    e_classes = sum(ent(L) for v in by_first.values() for L in v)
    out = dict(first_kmers=len(lists), classes=n_classes, classes_per_first_kmer=n_classes / max(len(lists), 1),
               list_len=dict(mean=float(lens.mean()), median=float(np.median(lens)), max=int(lens.max())),
               entries_without_classes=int(e_kmers), entries_with_classes=int(e_classes), entries_classes_ratio=e_classes / max(e_kmers, 1), caps={})
    for cap in caps:
        lim = cap if cap else 1 << 60
        groups = e_union = filt = filt_k = 0
        for v in by_first.values():
            cur, n_cls, n_km = set(), 0, 0

            def close():
                nonlocal groups, e_union, filt, filt_k
                if n_cls:
                    eu = ent(cur)
                    groups += 1; e_union += eu; filt += n_cls * eu; filt_k += n_km * eu
            for L in (sorted(v) if order == "list" else sorted(v, key=key_of)):
                k = v[L]
                while k:      # (a class of more than CLASS_CAP k-mers is cut, as the class finder cuts it)
                    if n_cls and (len(cur.union(L)) > lim or n_km >= CLASS_CAP):
                        close(); cur, n_cls, n_km = set(), 0, 0
                    take = min(k, CLASS_CAP - n_km)
                    cur.update(L); n_cls += 1; n_km += take; k -= take
            close()
        out["caps"][str(cap) if cap else "none"] = dict(
            groups=groups, classes_per_group=n_classes / max(groups, 1), first_kmers_per_group=len(lists) / max(groups, 1),
            union_entries=int(e_union), union_over_classes=e_union / max(e_classes, 1),
            filter_proxy_classes=filt / max(e_classes, 1), filter_proxy_first_kmers=filt_k / max(e_kmers, 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, action="append", default=[], help="reads of the bench's generator (n_units = 0.3 x reads); may repeat")
    ap.add_argument("--cenx", action="store_true", help="bench.py's CENX shape (workload_c)")
    ap.add_argument("--var-len", type=int, action="append", default=[], help="copy-specific variant length(s); default 8")
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--cap", type=int, action="append", default=[], help="cap(s) on the union's postings, 0 = none; default 32 64 0")
    ap.add_argument("--order", choices=("list", "second", "hash"), default="list", help="order of the k-mers of one first unit before the greedy cut")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    caps = a.cap or [32, 64, 0]
    P = bench.PARAMS
    runs = []
    for vl in a.var_len or [8]:
        for n in a.reads:
            runs.append((f"bench generator, {n} reads, seed {a.seed}, var_len {vl}", dict(bench.synth_kwargs(n, a.seed), n_reads=n, var_len=vl)))
        if a.cenx:
            runs.append((f"cenX shape ({bench.CENX['n_reads']} reads, {bench.CENX['n_units']} units), var_len {vl}", dict(bench.CENX, var_len=vl)))
    if not runs:
        ap.error("nothing to measure: --reads N and / or --cenx")
    res = []
    for name, kw in runs:
        m = measure(*clouds_of(kw), caps, max(P["min_d"], 1), P["max_d"], a.order)
        m["workload"] = name
        res.append(m)
        ll = m["list_len"]
        print(f"{name}\n  first k-mers {m['first_kmers']}  classes {m['classes']} ({m['classes_per_first_kmer']:.3f})  "
              f"entries with / without classes {m['entries_classes_ratio']:.3f}  list length mean {ll['mean']:.1f} median {ll['median']:.0f} max {ll['max']}")
        print("  cap    groups  classes/group  k-mers/group  union/classes  filter proxy (classes)  (first k-mers)")
        for c, g in m["caps"].items():
            print(f"  {c:>4} {g['groups']:9d} {g['classes_per_group']:14.1f} {g['first_kmers_per_group']:13.1f} {g['union_over_classes']:14.3f} "
                  f"{g['filter_proxy_classes']:23.2f} {g['filter_proxy_first_kmers']:16.2f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/dist_groups_cpu.py", params=dict(min_d=P["min_d"], max_d=P["max_d"]), runs=res), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Developer tool: what the waves of cf_group_walk_kernel do with their time, on the bench's workload.
usage: tools/walk_stamps.py --lib <a -DCF_WALK_STAMPS build> [--reads N] [--param knob=value ...]
       (tools/build_variant.sh walk_stamps -DCF_WALK_STAMPS makes such a build; --param dist_walk=0 measures the 256-thread kernel)
Runs one step of bench.py's reads (A1-A3, then one launch of the distance stage after a warm-up launch), reads the library's
"[cf_walk stamps]" line from stderr and prints the per-wave shader-clock sums and the two figures of DESIGN.md 36:
  cycles per member   = cycles inside the member loops / members walked
  share of slot time  = cycles inside the member loops / (workgroups' lifetimes x their waves): a wave's slot, its registers and its
                        share of the LDS are taken from its workgroup's start to the end of the workgroup's slowest wave."""
import argparse, json, os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload's parameters)
from centroflye_amd import _host, _lib  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--param", action="append", default=[])
    a = ap.parse_args()
    P = bench.PARAMS
    pk = _host.synth(n_reads=a.reads, **bench.synth_kwargs(a.reads, a.seed))
    e = Engine(0, _lib.load(os.path.abspath(a.lib)))
    for kv in a.param:
        e.set_param(kv.split("=")[0], int(kv.split("=")[1]))
    e.load(pk, 1); e.count_kmers(P["k"]); e.select_rare(P["max_nonuniq"], P["lo"], P["hi"]); e.build_clouds()
    args = (0, 2 ** 62, P["min_d"], P["max_d"], P["min_cov"], P["rel_threshold"], 0, 1, 0)
    e.dist_edges(*args)      # warm-up launch
    e.reset_unique()
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:      # the library writes its diagnostic lines to the C stderr
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            n_edges = e.dist_edges(*args)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    postings_ms = e.times()["postings_ms"]
    st = e.stats()
    e.close()
    m = re.search(r"\[cf_walk stamps\] (.*?) \(shader cycles summed over the waves of (\d+) workgroups; dist_walk=(\d)\)", text)
    if not m:
        sys.stderr.write(text)
        sys.exit("no [cf_walk stamps] line: is --lib a -DCF_WALK_STAMPS build?")
    c = {k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())}
    rec = dict(dist_walk=int(m.group(3)), workgroups=int(m.group(2)), postings_ms=round(postings_ms, 2), n_edges=int(n_edges), n_dist_passes=st["n_dist_passes"], **c)
    rec["cycles_per_member"] = round(c["member"] / max(1, c["members"]), 1)
    rec["postings_per_member"] = round(c["postings"] / max(1, c["members"]), 2)
    rec["member_share_of_slot_time"] = round(c["member"] / max(1, c["slot_life"]), 4)
    rec["load_share_of_slot_time"] = round(c["load"] / max(1, c["slot_life"]), 4)
    rec["wave_life_share_of_slot_time"] = round(c["wave_life"] / max(1, c["slot_life"]), 4)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

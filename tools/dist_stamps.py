#!/usr/bin/env python3
"""Developer tool: where thread 0 of cf_dist_kernel spends its time, phase by phase, on the bench's workload.
usage: tools/dist_stamps.py --lib <a -DCF_DIST_STAMPS build> [--reads N] [--param knob=value ...]
       (tools/build_variant.sh stamps -DCF_DIST_STAMPS makes such a build; a -DCF_DIST_DIAG_COUNT build given here has its
        "[cf_dist diag]" lines passed through instead — the two flags share counter words and do not go into one build)
Runs one step of bench.py's reads (A1-A3, then one launch of the distance stage after a warm-up launch), reads the library's
"[cf_dist stamps]" line from stderr and prints, per stamp, its share of thread 0's cycles and that share of the kernel's
milliseconds (device events).  The stamps are thread 0's view of every workgroup: a phase that thread 0 sits out at a
barrier is booked on the stamp behind that barrier."""
import argparse, json, os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload's parameters)
from centroflye_amd import _host, _lib  # noqa: E402
from centroflye_amd.engine import Engine  # noqa: E402

# the names the library prints, in kernel order, and what the stamp covers
STAMPS = [("pop", "0 queue pop, [top] barrier"), ("prologue", "1 prologue"), ("sketch", "6 sketch sweep (clear + own items)"),
          ("clear", "2 pop partition + clear table"), ("stream", "3 table sweep + inserts (own items)"),
          ("sweep_end_wait", "7 wait for the other waves at the end of a sweep"), ("filter", "4 filter (per member, to [filtered])"),
          ("write", "5 reserve + write rows")]


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
    ms = e.times()["dist_kernel_ms"]
    st = e.stats()
    e.close()
    for line in text.splitlines():
        if line.startswith("[cf_dist diag]"):
            print(line)
    m = re.search(r"\[cf_dist stamps\] (.*?) \(shader cycles summed over (\d+) workgroups; passes=(\d+)\)", text)
    if not m:
        sys.stderr.write(text)
        sys.exit("no [cf_dist stamps] line: is --lib a -DCF_DIST_STAMPS build?")
    cyc = {k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())}
    total = sum(cyc.values())
    print("dist_kernel_ms %.1f  workgroups %s  passes %s  edges %d  emissions %d" % (ms, m.group(2), m.group(3), n_edges, st["n_emissions"]))
    rec = dict(dist_kernel_ms=round(ms, 2), workgroups=int(m.group(2)), passes=int(m.group(3)), n_edges=int(n_edges), stamps={})
    for name, what in STAMPS:
        share = cyc.get(name, 0) / total if total else 0.0
        rec["stamps"][name] = dict(cycles=cyc.get(name, 0), share=round(share, 4), ms=round(share * ms, 2))
        print("%-15s %6.2f ms  %5.1f %%   %s" % (name, share * ms, 100 * share, what))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

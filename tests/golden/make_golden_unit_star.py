#!/usr/bin/env python3
"""Golden vectors for stage 4, the unit* reconstruction (scripts/better_consensus_unit_reconstruction.py:170-190
get_polished_unit, :193-212 main).  Runs the reference itself by import (build container only) with the real networkx; edlib is
a small ctypes module over edlibAlign of oracle/_ref/librr_ref.so (the reference's own vendored edlib, built by oracle/ref/Makefile),
Biopython a FASTA reader with SeqIO.parse's behaviour for the files used here.

The reference turns the top n into a set, so its graph's node order depends on PYTHONHASHSEED.  The goldens call its own
get_polished_unit with the top n as a LIST in descending (count, k-mer) order (heapq.nlargest's order), which is what the drop-in
does; main() itself is run under two (fixtures) or three (random cases) hash seeds and recorded with a hash_stable flag.

    python tests/golden/make_golden_unit_star.py            # writes <fixture>.unit_star.json and unit_star_cases.json
    PYTHONHASHSEED=7 python tests/golden/make_golden_unit_star.py --check
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/scripts"
LIBEDLIB = os.path.join(ROOT, "oracle", "_ref", "librr_ref.so")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("tiny", "lowcov", "hor2055", "exotic")
KS = (30, 19)
N_CASES = 44
SEEDS_FIXTURE = ("1", "2")
SEEDS_CASES = ("1", "2", "3")


# ---------------------------------------------------------------- stubs for the reference's imports
class _EdlibConfig(C.Structure):
    _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int), ("additionalEqualities", C.c_void_p),
                ("additionalEqualitiesLength", C.c_int)]


class _EdlibResult(C.Structure):
    _fields_ = [("status", C.c_int), ("editDistance", C.c_int), ("endLocations", C.POINTER(C.c_int)),
                ("startLocations", C.POINTER(C.c_int)), ("numLocations", C.c_int), ("alignment", C.c_void_p),
                ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]


def edlib_module():
    lib = C.CDLL(LIBEDLIB)
    lib.edlibAlign.restype = _EdlibResult
    lib.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _EdlibConfig]
    lib.edlibFreeAlignResult.argtypes = [_EdlibResult]
    modes, tasks = {"NW": 0, "SHW": 1, "HW": 2}, {"distance": 0, "locations": 1, "path": 2}

    def align(query, target, mode="NW", task="distance", k=-1):
        q, t = query.encode("latin-1"), target.encode("latin-1")
        r = lib.edlibAlign(q, len(q), t, len(t), _EdlibConfig(k, modes[mode], tasks[task], None, 0))
        locs = [(r.startLocations[i] if r.startLocations else None, r.endLocations[i]) for i in range(r.numLocations)]
        out = {"editDistance": r.editDistance, "alphabetLength": r.alphabetLength, "locations": locs, "cigar": None}
        lib.edlibFreeAlignResult(r)
        return out

    m = types.ModuleType("edlib")
    m.align = align
    return m


def bio_modules():
    class Rec:
        def __init__(self, title, seq):
            self.id = (title.split(None, 1) or [""])[0]
            self.seq = seq

    def parse(filename, format):
        if format != "fasta":
            raise ValueError(f"Unknown format '{format}'")
        with open(filename) as f:
            title, lines = None, []
            for ln in f:
                if ln[:1] == ">":
                    if title is not None:
                        yield Rec(title, "".join(lines).replace(" ", "").replace("\r", ""))
                    title, lines = ln[1:].rstrip(), []
                elif title is not None:
                    lines.append(ln.rstrip())
            if title is not None:
                yield Rec(title, "".join(lines).replace(" ", "").replace("\r", ""))

    bio, seqio = types.ModuleType("Bio"), types.ModuleType("Bio.SeqIO")
    seqio.parse = parse
    bio.SeqIO = seqio
    return bio, seqio


def import_reference():
    sys.dont_write_bytecode = True
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio_modules()
    sys.modules["edlib"] = edlib_module()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import better_consensus_unit_reconstruction as B
    from ncrf_parser import NCRF_Report
    return B, NCRF_Report


# ---------------------------------------------------------------- cases
def edit_unit(unit, rot, subs):
    """unit rotated left by rot, then substitutions [(position, base)]."""
    u = list(unit[rot:] + unit[:rot])
    for p, b in subs:
        u[p] = b
    return "".join(u)


def pick_edits(rng, unit, n_sub):
    rot = rng.randrange(1, len(unit))
    subs = []
    for p in rng.sample(range(len(unit)), n_sub):
        b = unit[(p + rot) % len(unit)]
        subs.append([p, rng.choice([c for c in "ACGT" if c != b.upper()])])
    return rot, subs


def ranked_top(B, rep, k, unit):
    counts, top = B.get_most_frequent_kmers(rep, k, unit)
    return counts, sorted(top, key=lambda x: (counts[x], x), reverse=True)


def graph_sizes(B, k, ranked, counts):
    """(nodes, edges) after the build, the first collapse, tips + second collapse and the purification (get_polished_unit's steps)."""
    g = B.DeBruijnGraph(k=k)
    g.add_kmers(ranked, "red", counts)
    out = [[g.graph.number_of_nodes(), g.graph.number_of_edges()]]
    g.collapse_nonbranching_paths()
    out.append([g.graph.number_of_nodes(), g.graph.number_of_edges()])
    g.remove_tips()
    g.collapse_nonbranching_paths()
    out.append([g.graph.number_of_nodes(), g.graph.number_of_edges()])
    g.purify_graph()
    out.append([g.graph.number_of_nodes(), g.graph.number_of_edges()])
    return out


def polished(B, k, ranked, counts, unit):
    try:
        return {"unit_star": B.get_polished_unit(k, ranked, counts, unit)}
    except Exception as e:      # the reference raises: the drop-in must refuse
        return {"error": type(e).__name__}


def top_digest(ranked, counts):
    return hashlib.sha256("".join(f"{x} {counts[x]}\n" for x in ranked).encode()).hexdigest()


# ---------------------------------------------------------------- main() under several hash seeds (child processes)
def child(job_fn):
    """Runs in a child process with its own PYTHONHASHSEED: the reference's main() per job, or get_polished_unit on a set."""
    B, _ = import_reference()
    with open(job_fn) as f:
        jobs = json.load(f)
    res = []
    for j in jobs:
        try:
            if j["kind"] == "main":
                sys.argv = ["better_consensus_unit_reconstruction.py", "--reads-ncrf", j["report"], "--unit", j["unit_fn"],
                            "-k", str(j["k"]), "--output", j["output"]]
                B.main()
                with open(j["output"], "rb") as f:
                    res.append(hashlib.sha256(f.read()).hexdigest())
            else:
                res.append(B.get_polished_unit(j["k"], set(j["kmers"]), dict(zip(j["kmers"], j["counts"])), j["unit"]))
        except Exception as e:
            res.append("error:" + type(e).__name__)
    print(json.dumps(res))


def run_children(jobs, seeds, wd):
    job_fn = os.path.join(wd, "jobs.json")
    with open(job_fn, "w") as f:
        json.dump(jobs, f)
    out = {}
    for s in seeds:
        env = dict(os.environ, PYTHONHASHSEED=s)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", job_fn], env=env, check=True,
                           capture_output=True, text=True)
        out[s] = json.loads(r.stdout.strip().splitlines()[-1])
    return out


# ---------------------------------------------------------------- fixtures
def fixture_golden(name, wd):
    import fixtures
    B, NCRF_Report = import_reference()
    report = fixtures.make_report(name, wd)
    rep = NCRF_Report(report)
    given = next(iter(rep.records.values())).motif
    rng = random.Random(f"unit_star/{name}")
    rot, subs = pick_edits(rng, given, 3)
    out = dict(fixture=name, report_sha256=fixtures.sha256_file(report), cases=[])
    jobs = []
    for k in KS:
        for edits in ([0, []], [rot, subs]):
            unit = edit_unit(given, *edits)
            counts, ranked = ranked_top(B, rep, k, unit)
            case = dict(k=k, rotation=edits[0], substitutions=edits[1], n=int(len({(unit + unit)[i:i + k] for i in range(len(unit))}) * 3),
                        n_top=len(ranked), top_digest=top_digest(ranked, counts), top_head=[[x, counts[x]] for x in ranked[:5]],
                        top_last=[ranked[-1], counts[ranked[-1]]] if ranked else None)
            case.update(polished(B, k, ranked, counts, unit))
            if "unit_star" in case:
                case["graph_sizes"] = graph_sizes(B, k, ranked, counts)
            out["cases"].append(case)
            unit_fn = os.path.join(wd, f"{name}_{k}_{edits[0]}.fasta")
            with open(unit_fn, "w") as f:
                f.write(f">unit\n{unit}\n")
            jobs.append(dict(kind="main", report=report, unit_fn=unit_fn, k=k, output=os.path.join(wd, f"o_{name}_{k}_{edits[0]}", "unit_star.fasta")))
    res = run_children(jobs, SEEDS_FIXTURE, wd)
    for i, case in enumerate(out["cases"]):
        case["main_sha256"] = {s: res[s][i] for s in SEEDS_FIXTURE}
        case["hash_stable"] = len(set(case["main_sha256"].values())) == 1
    return out


# ---------------------------------------------------------------- random cases
def case_params(i):
    rng = random.Random(1000 + i)
    unit_len = rng.choice([60, 90, 120, 150, 200, 240, 300])
    monomer_len = rng.choice([m for m in (20, 30, 50, 60) if unit_len % m == 0] or [unit_len])
    synth = dict(seed=5000 + i, unit_len=unit_len, monomer_len=monomer_len, n_units=max(rng.randrange(40, 90), 16000 // unit_len), flank=60000,
                 n_reads=rng.randrange(12, 30), mean_len=6500, sigma=0.2, min_len=6000, max_len=7000,
                 unit_div=rng.choice([0.0, 0.01, 0.03, 0.06, 0.12]), n_prefix=2, n_suffix=2, prefix_threshold=50000,
                 p_split=0.1, var_len=rng.choice([1, 1, 4]), n_threads=1)
    k = rng.choice([7, 9, 11, 15, 19, 23, 30])
    return synth, k, rng


def random_cases(wd):
    from centroflye_amd import _host
    B, NCRF_Report = import_reference()
    cases, jobs = [], []
    for i in range(N_CASES):
        synth, k, rng = case_params(i)
        report = os.path.join(wd, f"case{i}.ncrf")
        _host.synth(report_path=report, pack=False, **synth)
        rep = NCRF_Report(report)
        given = next(iter(rep.records.values())).motif
        mode = i % 3       # 0: the given unit, 1: rotated + substitutions, 2: rotated + many substitutions
        rot, subs = (0, []) if mode == 0 else pick_edits(rng, given, 2 if mode == 1 else max(3, len(given) // 15))
        unit = edit_unit(given, rot, subs)
        counts, ranked = ranked_top(B, rep, k, unit)
        case = dict(synth=synth, k=k, rotation=rot, substitutions=subs, n_top=len(ranked), top_digest=top_digest(ranked, counts))
        case.update(polished(B, k, ranked, counts, unit))
        cases.append(case)
        jobs.append(dict(kind="set", k=k, kmers=ranked, counts=[counts[x] for x in ranked], unit=unit))
    res = run_children(jobs, SEEDS_CASES, wd)
    for i, case in enumerate(cases):
        got = {res[s][i] for s in SEEDS_CASES}
        want = case.get("unit_star", "error:" + case.get("error", ""))
        case["hash_stable"] = got == {want}
    return dict(seeds=list(SEEDS_CASES), cases=cases)


def main():
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
        return
    check = "--check" in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(NAMES) + ["cases"]
    ok = True
    with tempfile.TemporaryDirectory() as wd:
        for name in names:
            if name == "cases":
                g, path = random_cases(wd), os.path.join(HERE, "unit_star_cases.json")
            else:
                g, path = fixture_golden(name, wd), os.path.join(HERE, f"{name}.unit_star.json")
            if check:
                with open(path) as f:
                    same = json.load(f) == json.loads(json.dumps(g))
                print(os.path.basename(path), "IDENTICAL" if same else "DIFFERENT")
                ok &= same
            else:
                with open(path, "w") as f:
                    json.dump(g, f, indent=1)
                    f.write("\n")
                print("wrote", path)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

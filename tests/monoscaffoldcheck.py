"""The inputs of tests/golden/mono_scaffold_cases.json and the functions that turn what a module set makes of them into records: shared
by tools/capture_mono_scaffold_cases.py (which runs them on the reference's modules) and tests/test_mono_scaffold.py and
tests/test_gpu_mono_scaffold.py (which run them on centroflye_amd's drop-ins and compare).  `mods` holds MonoString, split, ec
(mono_error_correction) and graph (debruijn_graph), as in tests/monographcheck.py, whose read records and shrinking are reused."""
import contextlib
import hashlib
import io
import json
import os
import random

import monographcheck as gc

GAP = "?"


def jkey(k):
    """a read id as a JSON object key"""
    return json.dumps(gc.key_json(k))


def tuples(x):
    """JSON lists back to the tuples the functions compare"""
    return tuple(tuples(y) for y in x) if isinstance(x, list) else x


def attempt(fn):
    """(result, None), or (None, the class of what it raised): a case where the reference raises records the class"""
    try:
        return fn(), None
    except Exception as e:      # noqa: BLE001 (the class is the record)
        return None, type(e).__name__


# ---------------------------------------------------------------- graphs
def graph_edges(mods, db):
    g = db.graph
    return list(g.edges(keys=True)) if getattr(mods, "networkx", False) else g.edges()


def edge_data(mods, db, e):
    return db.graph.get_edge_data(*e) if getattr(mods, "networkx", False) else db.graph.data(*e)


def edges_out(mods, db):
    """the edges in the order map_reads numbers them: [u, v, key, colour, sequence]"""
    return [[int(u), int(v), int(key), edge_data(mods, db, (u, v, key))["color"], edge_data(mods, db, (u, v, key))["edge_kmer"]] for u, v, key in graph_edges(mods, db)]


def build_db(mods, case, reads, tmp):
    """the graph of a case: add_kmers on the frequent k-mers of the reads with a small min_uniq_len, or the last graph of iterative_graph"""
    G = mods.graph
    if "iterative" in case:
        it = case["iterative"]
        with contextlib.redirect_stdout(io.StringIO()):
            _, dbs, _, _ = G.iterative_graph(reads, min_k=it["min_k"], max_k=it["max_k"], outdir=os.path.join(tmp, "idb_%s" % hashlib.sha1(case["name"].encode()).hexdigest()[:8]),
                                             min_mult=case["min_mult"])
        return dbs[it["max_k"]]
    strings = {r_id: ms.tostring() if hasattr(ms, "tostring") else "".join(ms.string) for r_id, ms in reads.items()}
    frequent, _ = G.get_frequent_kmers(strings, k=case["k"], min_mult=case["min_mult"])
    db = G.DeBruijnGraph(k=case["k"], min_uniq_len=case["min_uniq_len"])
    db.add_kmers(frequent, coverage=frequent)
    db.collapse_nonbranching_paths()
    return db


def hand_db(mods, spec):
    """a graph built edge by edge (k = 2: a node is a letter, an edge's string runs from its first node's letter to its last's):
    spec = [[u, v, colour, filler letters]]; the edges keep this order as long as it is sorted by first node"""
    db = mods.graph.DeBruijnGraph(k=2)
    for u, v, colour, filler in spec:
        seq = chr(65 + u) + filler + chr(65 + v)
        db.graph.add_edge(u, v, edge_kmer=seq, coverages=[1] * (len(seq) - 1), length=len(seq) - 1, color=colour)
    return db


def make_reads(mods, case):
    """{id: MonoString}; a record [name, text, strand, min_length] is cut at its gaps by split, its parts keyed (name, part)"""
    reads = {}
    for rec in case["reads"]:
        ms = gc.make_read(mods, rec[:3])
        if len(rec) > 3:
            with contextlib.redirect_stdout(io.StringIO()):
                reads.update(mods.split(ms, GAP, rec[3]))
        else:
            reads[rec[0]] = ms
    return reads


def mapping_out(mapping):
    out = {}
    for r_id, m in mapping.items():
        if m is None:
            out[jkey(r_id)] = None
        else:
            ((e0, j0), i0), ((e1, j1), i1), valid, path = m
            out[jkey(r_id)] = [[int(e0), int(j0), int(i0)], [int(e1), int(j1), int(i1)], bool(valid), [[int(x) for x in e] for e in path]]
    return out


# ---------------------------------------------------------------- the pipeline cases: reads -> graph -> mapping -> scaffolds -> pseudounits
U1, U2, U3, REP = "ABCDEFGHIJ", "KLMNOPQRST", "UVWabcdefg", "XYZ"
GENOME = U1 + REP + U2 + REP + U3


def tiled(text, length, step, prefix, times=1):
    return [gc.read_record("%s%02d_%d" % (prefix, x, t), text[a:a + length]) for x, a in enumerate(range(0, len(text) - length + 1, step)) for t in range(times)]


def pipeline_cases(rng):
    base = tiled(GENOME, 18, 2, "r", 2)
    extra = [gc.read_record("inrep", "XYZ"), gc.read_record("short", "AB"), gc.read_record("alien", "hijklmn"), gc.read_record("empty", ""),
             gc.read_record("del", GENOME[:4] + GENOME[5:12]), gc.read_record("jump", U1[2:9] + U3[1:8]), gc.read_record("gap", U1[:4] + "?" + U1[5:] + REP + U2[:5]),
             gc.read_record("minus", GENOME[3:20], True), ["cut", GENOME[2:11] + "?" + GENOME[12:24] + "?" + GENOME[14:34], "+", 4],
             ["cutm", GENOME[1:9] + "?" + GENOME[10:26], "-", 3]]
    noisy = []
    for x in range(40):
        a = rng.randrange(0, len(GENOME) - 16)
        text = list(GENOME[a:a + rng.randrange(10, 22)])
        if x % 5 == 0:
            text[rng.randrange(len(text))] = GAP
        if x % 7 == 0:
            text[rng.randrange(len(text))] = rng.choice("ABCXYZ")
        noisy.append(gc.read_record("n%02d" % x, "".join(text), x % 4 == 3))
    hor = {"h%02d" % x: gc.hor_text(rng, gc.HOR12, 9, subs=1, dels=0, gaps=0.01, phase=x % 12, variant=(4, 5, "X") if x % 2 else None) for x in range(30)}
    return [
        dict(name="three long edges joined through a repeat; reads that fit one place, two places, none; cut reads", reads=base + extra, k=3, min_mult=2, min_uniq_len=8,
             min_connections=2),
        dict(name="the same at k = 4 with min_connections 1 and noisy reads", reads=base + noisy, k=4, min_mult=2, min_uniq_len=8, min_connections=1),
        dict(name="nothing long: no scaffold at all", reads=base + extra, k=3, min_mult=2, min_uniq_len=1000, min_connections=2),
        dict(name="a graph of iterative_graph on a 12-letter HOR with a variant monomer", reads=[gc.read_record(n, t) for n, t in hor.items()], min_mult=2,
             iterative=dict(min_k=4, max_k=7), min_connections=2),
    ]


def run_pipeline(mods, case, tmp, raw=False):
    """raw: the values as they are (the capturing tool looks at them before it shrinks them)"""
    shrink_all = (lambda w: w) if raw else gc.shrink_all
    G = mods.graph
    reads = make_reads(mods, case)
    db = build_db(mods, case, reads, tmp)
    k = db.k
    want = {"edges": edges_out(mods, db), "reads": sorted(jkey(r) for r in reads)}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mapping, err = attempt(lambda: db.map_reads(reads, verbose=True))
    want["map_reads"] = mapping_out(mapping) if err is None else {"raises": err}
    want["printed"] = out.getvalue()
    index, ierr = attempt(lambda: db.index_edges())
    want["index_edges"] = {str(kk): sorted([kmer, list(at)] for kmer, at in v.items()) for kk, v in index.items()} if ierr is None else {"raises": ierr}
    if err is not None:
        return shrink_all(want)
    (res, err) = attempt(lambda: G.scaffolding(db, mapping, min_connections=case["min_connections"]))
    if err is not None:
        want["scaffolding"] = {"raises": err}
        return shrink_all(want)
    scaffolds, edge_scaffolds = res
    want["scaffolding"] = {"scaffolds": scaffolds, "edge_scaffolds": [[[int(x) for x in e] for e in s] for s in edge_scaffolds]}
    r2s, err = attempt(lambda: G.read2scaffolds(db, edge_scaffolds, mapping, reads))
    want["read2scaffolds"] = {jkey(r): [int(x) for x in at] for r, at in r2s.items()} if err is None else {"raises": err}
    if err is not None:
        return shrink_all(want)
    cov, err = attempt(lambda: G.cover_scaffolds_w_reads(r2s, mapping, scaffolds, reads, k))
    want["cover_scaffolds_w_reads"] = [[{jkey(r): [m, int(st), int(en)] for r, (m, st, en) in at.items()} for at in s] for s in cov] if err is None else {"raises": err}
    if err is not None:
        return shrink_all(want)
    want["partition_pseudounits"] = [[list(u) for u in G.partition_pseudounits(s)] for s in scaffolds]
    for min_cov in (0, 2):
        res, err = attempt(lambda: G.extract_read_pseudounits(cov, scaffolds, reads, min_coverage=min_cov))
        want["extract_read_pseudounits_%d" % min_cov] = {"raises": err} if err is not None else {
            "pseudounits": [[list(u) for u in s] for s in res[0]],
            "read_pseudounits": [[{jkey(r): [int(st), int(en), strand] for r, (st, en, strand) in unit.items()} for unit in s] for s in res[1]]}
    return shrink_all(want)


# ---------------------------------------------------------------- scaffolding alone, on hand-built graphs and mappings
def scaffolding_cases():
    B, K = "blue", "black"
    chain = [[0, 1, B, "aa"], [1, 2, K, ""], [2, 3, B, "bb"], [3, 4, K, "c"], [4, 5, B, "dd"], [5, 7, K, "r"], [5, 8, K, "rr"], [6, 0, K, "l"], [9, 6, K, "ll"]]
    L0, s1, L1, s2, L2, y, y2, x, x2 = range(9)
    two_ways = [[0, 1, B, "aa"], [1, 2, K, "p"], [1, 2, K, "q"], [2, 3, B, "bb"]]
    diamond = [[0, 1, B, "a"], [1, 2, B, "b"], [1, 3, B, "c"], [2, 4, B, "d"], [3, 4, B, "e"], [4, 5, B, "f"]]
    cyc = [[0, 1, B, "a"], [1, 0, B, "b"], [2, 3, B, "c"], [3, 4, B, "d"], [5, 6, B, "e"]]
    many = [[2 * c, 2 * c + 1, B, "a"] for c in range(7)] + [[2 * c + 1, 2 * c + 2, B, "b"] for c in (0, 2, 4)]
    many.sort(key=lambda e: e[0])
    return [
        dict(name="a chain of three long edges; left and right extensions, the longest wins, the first of equal ones stays", graph=chain, min_connections=2,
             mappings=[[True, [L0, s1, L1]], [True, [L0, s1, L1]], [True, [L1, s2, L2]], [True, [x, L0, s1, L1, s2, L2, y]], [True, [x2, x, L0]], [True, [L2, y2]], [True, [L2, y]], None,
                       [False, [x2, x, L0, s1, L1, s2, L2, y2, y]]]),
        dict(name="min_connections met by exactly two reads", graph=chain, min_connections=2, mappings=[[True, [L0, s1, L1]], [True, [L0, s1, L1]], [True, [L1, s2, L2]]]),
        dict(name="min_connections 1 links what one read supports", graph=chain, min_connections=1, mappings=[[True, [L0, s1, L1]], [True, [L0, s1, L1]], [True, [L1, s2, L2]]]),
        dict(name="min_connections 3 is missed by two reads", graph=chain, min_connections=3, mappings=[[True, [L0, s1, L1]], [True, [L0, s1, L1]], [True, [L1, s2, L2]]]),
        dict(name="invalid paths and reads without a hit count for nothing", graph=chain, min_connections=1, mappings=[[False, [L0, s1, L1]], None, [True, [L1, s2, L2]], [False, [x, L1]]]),
        dict(name="two connections with equal support: the first one found fills the link", graph=two_ways, min_connections=2,
             mappings=[[True, [0, 2, 3]], [True, [0, 1, 3]], [True, [0, 1, 3]], [True, [0, 2, 3]]]),
        dict(name="the better supported connection fills the link", graph=two_ways, min_connections=2, mappings=[[True, [0, 2, 3]], [True, [0, 1, 3]], [True, [0, 2, 3]]]),
        dict(name="additional_edges: a black edge as an anchor", graph=chain, min_connections=1, additional=[s1],
             mappings=[[True, [L0, s1, L1]], [True, [s1, L1, s2, L2]], [True, [L1, s2, L2]]]),
        dict(name="ties in the longest path: a diamond, predecessors in the order of their edges", graph=diamond, min_connections=1,
             mappings=[[True, [0, 2]], [True, [0, 1]], [True, [1, 3]], [True, [2, 4]], [True, [4, 5]], [True, [3, 5]]]),
        dict(name="the same diamond with the other side first", graph=diamond, min_connections=1,
             mappings=[[True, [0, 1]], [True, [0, 2]], [True, [2, 4]], [True, [1, 3]], [True, [3, 5]], [True, [4, 5]]]),
        dict(name="a fork: two ends equally far", graph=diamond, min_connections=1, mappings=[[True, [0, 2]], [True, [0, 1]]]),
        dict(name="a cyclic component is skipped, its neighbours are not", graph=cyc, min_connections=1, mappings=[[True, [0, 1]], [True, [1, 0]], [True, [2, 3]]]),
        dict(name="a read that passes an anchor twice", graph=cyc, min_connections=1, mappings=[[True, [0, 1, 0]], [True, [2, 3]], [True, [2, 3]]]),
        dict(name="many small components: each smaller than half the graph", graph=many, min_connections=1,
             mappings=[[True, [many.index([2 * c, 2 * c + 1, B, "a"]), many.index([2 * c + 1, 2 * c + 2, B, "b"]), many.index([2 * c + 2, 2 * c + 3, B, "a"])]] for c in (4, 0, 2)]),
        dict(name="no mapping at all: every long edge is its own scaffold", graph=chain, min_connections=2, mappings=[]),
        dict(name="no long edge", graph=[[0, 1, K, "a"], [1, 2, K, "b"]], min_connections=1, mappings=[[True, [0, 1]]]),
    ]


def run_scaffolding(mods, case):
    db = hand_db(mods, case["graph"])
    edges = graph_edges(mods, db)
    assert [list(e[:2]) for e in edges] == [e[:2] for e in case["graph"]], "the hand-built edges are not in edges() order"
    mappings = {}
    for x, m in enumerate(case["mappings"]):
        mappings["q%d" % x] = None if m is None else (((m[1][0], 0), 0), ((m[1][-1], 0), 0), m[0], [edges[e] for e in m[1]])
    res, err = attempt(lambda: mods.graph.scaffolding(db, mappings, min_connections=case["min_connections"], additional_edges=[edges[e] for e in case.get("additional", [])]))
    if err is not None:
        return {"raises": err}
    return {"scaffolds": res[0], "edge_scaffolds": [[edges.index(tuple(e)) for e in s] for s in res[1]]}


# ---------------------------------------------------------------- pseudounits of literal strings
PARTITION_STRINGS = ["", "A", "AA", "ABCABC", "ABCDA", "ABACABAD", "ABCDEFGHIJKLABCDEFGHIJKL", "AB?AB??", "ABCCBA", "ABCDEFXGHIJKLABCDEF"]


def run_partition(mods):
    return [[s, [list(u) for u in mods.graph.partition_pseudounits(s)]] for s in PARTITION_STRINGS]


# ---------------------------------------------------------------- end to end: decomposition.tsv -> the five files of the driver
E2E = dict(seed=33, n_reads=40, array_units=200, read_units=75, gaps=0.004, subs=0.001, k=40, min_mult=3, repeat=(66, 134, 4))


def e2e_inputs(spec=E2E):
    """(monomers.fasta text, decomposition.tsv text): reads of a planted array of the 18-letter HOR in which every unit carries another
    monomer at position 7 — so that every window of two units is unique and the default graph parameters see long unique edges — but
    for `repeat` = (unit a, unit b, n): the n units from b repeat those from a, which joins three long edges through a repeat"""
    rng = random.Random(spec["seed"])
    names = ["D6Z1_m%02d" % x for x in range(18)]
    fasta = "".join(">%s\n%s\n" % (n, "ACGT" * 42 + "AC"[:x % 3]) for x, n in enumerate(names))
    others = [c for c in gc.D6Z1 if c != gc.D6Z1[7]]
    pairs = [(a, b) for a in others for b in others]
    rng.shuffle(pairs)
    letters, seen = [rng.choice(others)], set()
    while len(letters) < spec["array_units"]:      # a walk on which no pair of neighbouring variants comes twice
        nxt = [b for a, b in pairs if a == letters[-1] and (a, b) not in seen]
        b = nxt[0] if nxt else rng.choice(others)
        seen.add((letters[-1], b))
        letters.append(b)
    a, b, n = spec["repeat"]
    letters[b:b + n] = letters[a:a + n]
    array = []
    for u in range(spec["array_units"]):
        unit = list(gc.D6Z1)
        unit[7] = letters[u]
        array += unit
    rows = []
    for q in range(spec["n_reads"]):
        r_id = "read_%02d" % q
        top = spec["array_units"] - spec["read_units"]      # (every eighth read starts at the array's first letter, the next one ends at its last)
        start = 0 if q % 8 == 0 else 18 * top if q % 8 == 1 else 18 * rng.randrange(0, top) + rng.randrange(0, 18) * (q % 2)
        seq = array[start:start + 18 * spec["read_units"]]
        minus = q % 3 == 2
        order = seq[::-1] if minus else seq
        for x, c in enumerate(order):
            shown = rng.choice(gc.D6Z1) if rng.random() < spec["subs"] else c
            rel = "?" if rng.random() < spec["gaps"] else "+"
            rows.append("%s\t%s%s\t%d\t%d\t%.2f\t%s\n" % (r_id, names[ord(shown) - 65], "'" if minus else "", 171 * x, 171 * x + 169, 92.5, rel))
    return fasta, "".join(rows)


FILES = ("ec_monostrings.tsv", "idb/contigs.tsv", "idb/edges.tsv", "mappings.tsv", "scaffolds.tsv", "pseudounits.tsv", "read_pseudounits.tsv")


def file_record(text):
    return {"sha1": hashlib.sha1(text.encode()).hexdigest(), "bytes": len(text), "lines": text.count("\n")}


def e2e_args(tmp, stop_after, spec=E2E):
    return ["--sd-report", os.path.join(tmp, "decomposition.tsv"), "--monomers", os.path.join(tmp, "monomers.fasta"), "--centromeric-reads",
            os.path.join(tmp, "reads.fasta"), "--outdir", os.path.join(tmp, "out_%s" % stop_after), "--min-k", str(spec["k"]), "--max-k", str(spec["k"]),
            "--min-mult", str(spec["min_mult"])] + ([] if stop_after == "none" else ["--stop-after", stop_after])


def write_e2e_inputs(tmp, spec=E2E):
    fasta, tsv = e2e_inputs(spec)
    for name, text in (("monomers.fasta", fasta), ("decomposition.tsv", tsv), ("reads.fasta", ">unused\nACGT\n")):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)


def listed(outdir):
    return sorted(os.path.relpath(os.path.join(d, f), outdir) for d, _, fs in os.walk(outdir) for f in fs)


def check_end_to_end(tmp, golden):
    """the driver's main on the generated report: --stop-after pseudounits writes the files the reference's own calls give, mapping and
    scaffolds write their prefixes, and without --stop-after it refuses and writes nothing"""
    import pytest
    from centroflye_amd import centroflye_mono
    assert golden["spec"] == json.loads(json.dumps(E2E))
    tmp = str(tmp)
    write_e2e_inputs(tmp)
    prefixes = {"mapping": FILES[:4], "scaffolds": FILES[:5], "pseudounits": FILES}
    for stop in ("pseudounits", "mapping", "scaffolds"):
        with contextlib.redirect_stdout(io.StringIO()):
            assert centroflye_mono.main(e2e_args(tmp, stop)) == 0
        out = os.path.join(tmp, "out_%s" % stop)
        assert listed(out) == sorted(prefixes[stop])
        for name in prefixes[stop]:
            with open(os.path.join(out, name)) as f:
                assert file_record(f.read()) == golden["files"][name], (stop, name)
    with pytest.raises(SystemExit) as e:
        centroflye_mono.main(e2e_args(tmp, "none"))
    assert "polishing" in str(e.value.code) and not os.path.exists(os.path.join(tmp, "out_none"))

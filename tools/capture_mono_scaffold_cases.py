#!/usr/bin/env python3
"""Developer tool (BUILD CONTAINER ONLY: needs the reference checkout with networkx and pandas, no GPU): captures what the reference's
scripts/debruijn_graph.py makes of small inputs behind the graph — map_reads, index_edges, scaffolding, read2scaffolds,
cover_scaffolds_w_reads, partition_pseudounits, extract_read_pseudounits — into tests/golden/mono_scaffold_cases.json, the fixture
that pins those functions of centroflye_amd/debruijn_graph.py and the driver's files (tests/test_mono_scaffold.py,
tests/test_gpu_mono_scaffold.py).  The reference's modules are imported as they are, with Bio.SeqIO and networkx's
nx_pydot.write_dot stubbed; nothing of them is copied.  The file holds inputs and recorded results only; long values as length +
SHA-1.  The case inputs and the record format are in tests/monoscaffoldcheck.py.

The tool fails unless the reference's own results show what the cases are there for: a scaffold of two or more long edges, a left
and a right extension, a read that maps to exactly one place of a scaffold, a pseudounit covered by two or more reads, and an
end-to-end input with a scaffold and a covered pseudounit.  The order of a set of edge tuples shapes the reference's scaffolds, so
the tool runs the capture in three child processes under PYTHONHASHSEED = 0, 1 and 12345 and fails unless the three files are equal
byte by byte.
usage: tools/capture_mono_scaffold_cases.py [--reference DIR] [--seed S] [--out FILE]"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import monoscaffoldcheck as sc  # noqa: E402  (the case inputs and the record format are shared with the tests)


def arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    ref = os.path.join(arg("--reference", "/root/reference"), "scripts")
    out_fn = arg("--out", os.path.join(ROOT, "tests", "golden", "mono_scaffold_cases.json"))
    if not os.path.isdir(ref):
        sys.exit("this tool needs the reference checkout (--reference DIR; build container only)")
    sys.dont_write_bytecode = True
    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, bio.SeqIO
    import networkx
    networkx.drawing.nx_pydot.write_dot = lambda graph, path: None
    sys.path.insert(0, ref)
    import debruijn_graph as RG
    import mono_error_correction as RE
    import sd_parser as RP
    rng = random.Random(arg("--seed", 33, int))
    mods = types.SimpleNamespace(MonoString=RP.MonoString, split=lambda ms, c, n: ms.split(c, n), ec=RE, graph=RG, networkx=True)
    out = {"source": "scripts/debruijn_graph.py of the reference (with scripts/sd_parser.py and scripts/mono_error_correction.py in front of it), captured by "
                     "tools/capture_mono_scaffold_cases.py (networkx %s)" % networkx.__version__}
    with warnings.catch_warnings(), tempfile.TemporaryDirectory() as tmp:
        warnings.simplefilter("ignore")
        from monographcheck import shrink_all
        raws = [(case, sc.run_pipeline(mods, case, tmp, raw=True)) for case in sc.pipeline_cases(rng)]
        out["pipeline"] = [dict(case, want=shrink_all(raw)) for case, raw in raws]
        out["scaffolding"] = [dict(case, want=sc.run_scaffolding(mods, case)) for case in sc.scaffolding_cases()]
        out["partition"] = sc.run_partition(mods)

        # what the cases are there for, on the reference's own results
        hand = [c for c in out["scaffolding"] if "raises" not in c["want"] and "additional" not in c]
        colour = lambda c, e: c["graph"][e][2]      # noqa: E731
        assert any(sum(colour(c, e) == "blue" for e in s) >= 2 for c in hand for s in c["want"]["edge_scaffolds"]), "no scaffold of two long edges"
        assert any(colour(c, s[0]) == "black" for c in hand for s in c["want"]["edge_scaffolds"]), "no left extension"
        assert any(colour(c, s[-1]) == "black" for c in hand for s in c["want"]["edge_scaffolds"]), "no right extension"
        assert any(raw.get("read2scaffolds") and "raises" not in raw["read2scaffolds"] for _, raw in raws), "no read maps to exactly one place"
        assert any(len(unit) >= 2 for _, raw in raws for s in raw.get("extract_read_pseudounits_0", {}).get("read_pseudounits", []) for unit in s), \
            "no pseudounit is covered by two reads"
        assert any(m is None for _, raw in raws for m in raw["map_reads"].values()) and any(m is not None and not m[2] for _, raw in raws for m in raw["map_reads"].values())
        assert any(row[3] == "blue" for _, raw in raws for row in raw["edges"])

        # end to end: the reference's own calls on the generated report; the files are in this project's format (centroflye_amd/centroflye_mono.py)
        from centroflye_amd import centroflye_mono as drv
        sc.write_e2e_inputs(tmp)
        import Bio.SeqIO

        def parse(filename, format=None):
            with open(filename) as f:
                for block in f.read().split(">")[1:]:
                    head, _, seq = block.partition("\n")
                    yield types.SimpleNamespace(id=head.split()[0], seq=seq.replace("\n", ""))
        Bio.SeqIO.parse = parse
        k, spec = sc.E2E["k"], sc.E2E
        with contextlib.redirect_stdout(io.StringIO()):
            report = RP.SD_Report(os.path.join(tmp, "decomposition.tsv"), os.path.join(tmp, "monomers.fasta"))
            ec = RE.error_correction(report.monostrings, verbose=True, inplace=False)
            contigs, dbs, _, _ = RG.iterative_graph(ec, min_k=k, max_k=k, outdir=os.path.join(tmp, "idb"), min_mult=spec["min_mult"])
            db = dbs[k]
            mappings = db.map_reads(ec, verbose=False)
            scaffolds, edge_scaffolds = RG.scaffolding(db, mappings)
            r2s = RG.read2scaffolds(db, edge_scaffolds, mappings, ec)
            coverage = RG.cover_scaffolds_w_reads(r2s, mappings, scaffolds, ec, k=db.k)
            pseudounits, read_pseudounits = RG.extract_read_pseudounits(coverage, scaffolds, monostrings=ec)
        db_edges = list(db.graph.edges(keys=True))
        edge_index = {e: x for x, e in enumerate(db_edges)}
        datas = [db.graph.get_edge_data(*e) for e in db_edges]
        texts = {
            "ec_monostrings.tsv": drv.ec_lines(ec), "idb/contigs.tsv": drv.contig_lines(contigs),
            "idb/edges.tsv": drv.edge_lines([e + (d["color"], d["coverages"], d["edge_kmer"]) for e, d in zip(db_edges, datas)]),
            "mappings.tsv": drv.mapping_lines(mappings, edge_index), "scaffolds.tsv": drv.scaffold_lines(scaffolds, edge_scaffolds, edge_index),
            "pseudounits.tsv": drv.pseudounit_lines(pseudounits, read_pseudounits), "read_pseudounits.tsv": drv.read_pseudounit_lines(read_pseudounits)}
        assert set(texts) == set(sc.FILES)
        n_long = sum(d["color"] == "blue" for d in datas)
        covered = sum(len(unit) >= 1 for s in read_pseudounits for unit in s)
        print("end to end: %d reads, %d edges (%d long; lengths %s), %d scaffolds, %d placed reads, %d covered pseudounits" % (
            len(ec), len(db_edges), n_long, sorted(len(d["edge_kmer"]) for d in datas)[-6:], len(scaffolds), len(r2s), covered))
        assert len(scaffolds) >= 1 and covered >= 1 and n_long >= 1, "the end-to-end input yields no scaffold or no covered pseudounit"
        out["e2e"] = dict(spec=spec, files={name: sc.file_record("".join(lines)) for name, lines in texts.items()},
                          figures=dict(edges=len(db_edges), long_edges=n_long, scaffolds=len(scaffolds), long_edges_per_scaffold=[sum(datas[edge_index[e]]["color"] == "blue" for e in s)
                                                                                                                          for s in edge_scaffolds],
                                       reads=len(ec), mapped=sum(m is not None for m in mappings.values()), valid=sum(m is not None and m[2] for m in mappings.values()),
                                       placed=len(r2s), pseudounits=sum(map(len, pseudounits)), covered_pseudounits=covered,
                                       covered_by_two=sum(len(unit) >= 2 for s in read_pseudounits for unit in s)))
        print("end to end:", out["e2e"]["figures"])
    with open(out_fn, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d pipeline, %d scaffolding cases, %d bytes -> %s" % (len(out["pipeline"]), len(out["scaffolding"]), os.path.getsize(out_fn), out_fn))
    print("cases that raise:", [c["name"] for c in out["scaffolding"] if "raises" in c["want"]],
          [(c["name"], key) for c in out["pipeline"] for key, v in c["want"].items() if isinstance(v, dict) and "raises" in v])


HASH_SEEDS = ("0", "1", "12345")


def three_seeds():
    """the capture in three child processes under different PYTHONHASHSEEDs: the files have to be equal byte by byte"""
    import subprocess
    out_fn = arg("--out", os.path.join(ROOT, "tests", "golden", "mono_scaffold_cases.json"))
    rest = [a for x, a in enumerate(sys.argv[1:]) if a != "--out" and sys.argv[x] != "--out"]
    with tempfile.TemporaryDirectory() as tmp:
        texts = []
        for seed in HASH_SEEDS:
            fn = os.path.join(tmp, "cases_%s.json" % seed)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", fn] + rest, env=dict(os.environ, PYTHONHASHSEED=seed),
                               capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("PYTHONHASHSEED=%s: the capture failed\n%s%s" % (seed, r.stdout[-2000:], r.stderr[-4000:]))
            with open(fn, "rb") as f:
                texts.append(f.read())
        if any(t != texts[0] for t in texts[1:]):
            sys.exit("the captured files differ between PYTHONHASHSEED = %s: an order of the reference's is not pinned" % ", ".join(HASH_SEEDS))
        sys.stdout.write(r.stdout)
        with open(out_fn, "wb") as f:
            f.write(texts[0])
    print("equal under PYTHONHASHSEED = %s -> %s" % (", ".join(HASH_SEEDS), out_fn))


if __name__ == "__main__":
    main() if "--child" in sys.argv else three_seeds()

#!/usr/bin/env python3
"""Developer tool (BUILD CONTAINER ONLY: needs the reference checkout with networkx and pandas, no GPU): captures what the reference's
scripts/sd_parser.py (MonoString.split), scripts/mono_error_correction.py and scripts/debruijn_graph.py make of small inputs into
tests/golden/mono_graph_cases.json, the fixture that pins centroflye_amd/mono_error_correction.py (split_monostring included) and
centroflye_amd/debruijn_graph.py (tests/test_mono_graph.py).  The reference's modules are imported as they are, with Bio.SeqIO and
networkx's nx_pydot.write_dot stubbed; nothing of them is copied.  The file holds inputs and recorded results only.

Sections: "split" (the strings of the issue, seeded random strings with min_length 1 .. 6, forward and reversed reads; the raised
exception's class where the reference raises), "correction" (each of the five steps on its own and error_correction whole with its
printed lines; string, strand and mono2nucl per output key, in output order), "graph" (get_frequent_kmers with its order and
positions, the collapsed edges, get_edges, get_contigs with its paths as sequences, get_edgepath2coords, get_long_edges,
get_paths_thru_complex_nodes) and "iterative" (iterative_graph: the contigs and frequent k-mers of every k, the printed lines).
usage: tools/capture_mono_graph_cases.py [--reference DIR] [--seed S]"""
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
OUT = os.path.join(ROOT, "tests", "golden", "mono_graph_cases.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import monographcheck as gc  # noqa: E402  (the case inputs and the record format are shared with the test)


def arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    ref = os.path.join(arg("--reference", "/root/reference"), "scripts")
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
    rng = random.Random(arg("--seed", 29, int))
    mods = types.SimpleNamespace(MonoString=RP.MonoString, split=lambda ms, c, n: ms.split(c, n), ec=RE, graph=RG, networkx=True)
    out = {"source": "scripts/sd_parser.py (MonoString.split), scripts/mono_error_correction.py and scripts/debruijn_graph.py of the reference, "
                     "captured by tools/capture_mono_graph_cases.py (networkx %s)" % networkx.__version__}
    with warnings.catch_warnings(), tempfile.TemporaryDirectory() as tmp:
        warnings.simplefilter("ignore")
        out["split"] = [dict(case, want=gc.run_split(mods, case)) for case in gc.split_cases(rng)]
        out["correction"] = [dict(case, want=gc.run_correction(mods, case)) for case in gc.correction_cases(rng)]
        out["graph"] = [dict(case, want=gc.run_graph(mods, case)) for case in gc.graph_cases(rng)]
        out["iterative"] = [dict(case, want=gc.run_iterative(mods, case, tmp)) for case in gc.iterative_cases(rng)]
        # end to end: the reference on the generated report; the two files are in this project's format (centroflye_amd/centroflye_mono.py)
        from centroflye_amd import centroflye_mono
        fasta, tsv, truth = gc.e2e_inputs()
        with open(os.path.join(tmp, "m.fasta"), "w") as f:
            f.write(fasta)
        with open(os.path.join(tmp, "d.tsv"), "w") as f:
            f.write(tsv)
        import Bio.SeqIO

        def parse(filename, format=None):
            with open(filename) as f:
                for block in f.read().split(">")[1:]:
                    head, _, seq = block.partition("\n")
                    yield types.SimpleNamespace(id=head.split()[0], seq=seq.replace("\n", ""))
        Bio.SeqIO.parse = parse
        with contextlib.redirect_stdout(io.StringIO()) as printed:
            report = RP.SD_Report(os.path.join(tmp, "d.tsv"), os.path.join(tmp, "m.fasta"))
            before = {r: ms.tostring() for r, ms in report.monostrings.items()}
            ec = RE.error_correction(report.monostrings, verbose=True, inplace=False)
            contigs, _, _, _ = RG.iterative_graph(ec, min_k=gc.E2E["min_k"], max_k=gc.E2E["max_k"], outdir=os.path.join(tmp, "idb"), min_mult=gc.E2E["min_mult"])
        out["e2e"] = dict(spec=gc.E2E, want=gc.e2e_files("".join(centroflye_mono.ec_lines(ec)), "".join(centroflye_mono.contig_lines(contigs)), before, truth),
                          printed=printed.getvalue())
        print("end to end:", {k: v for k, v in out["e2e"]["want"].items() if k != "contigs"})
    with open(OUT, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d split, %d correction, %d graph, %d iterative cases, %d bytes -> %s" % (
        len(out["split"]), len(out["correction"]), len(out["graph"]), len(out["iterative"]), os.path.getsize(OUT), OUT))
    print("split cases that raise:", sum("raises" in c["want"] for c in out["split"]))
    print("iterative cases that raise:", [c["name"] for c in out["iterative"] if "raises" in c["want"]])


if __name__ == "__main__":
    main()

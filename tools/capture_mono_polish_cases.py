#!/usr/bin/env python3
"""Developer tool (BUILD CONTAINER ONLY: needs the reference checkout with networkx and pandas, no GPU): captures what the reference's
``polish`` (scripts/debruijn_graph.py) writes and prints for the cases of tests/monopolishcheck.py into
tests/golden/mono_polish_cases.json, the fixture that pins centroflye_amd.debruijn_graph.polish (tests/test_mono_polish.py).  The
reference's module is imported as it is, with Bio.SeqIO stubbed; nothing of it is copied.  In Flye's place runs a stub program of
this project, written to a temporary directory, that copies template.fasta to polished_N.fasta.  The file holds the inputs, the text
of every reads.fasta, template.fasta, polished_N.fasta and scaffold_i.fasta, and the printed command lines (the run's two paths
replaced by OUTDIR and FLYE).

The tool fails unless the cases show what they are there for: both strands, lower case and N in a read, (id, part) keys, two
scaffolds, an even number of reads, a template chosen by sorted order against dict order, and a duplicate segment id.
usage: tools/capture_mono_polish_cases.py [--reference DIR] [--out FILE]"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import monopolishcheck as mp  # noqa: E402  (the cases and the record format are shared with the tests)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    ref = os.path.join(arg("--reference", "/root/reference"), "scripts")
    out_fn = arg("--out", os.path.join(ROOT, "tests", "golden", "mono_polish_cases.json"))
    if not os.path.isdir(ref):
        sys.exit("this tool needs the reference checkout (--reference DIR; build container only)")
    sys.dont_write_bytecode = True
    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")

    def parse(filename, format=None):
        with open(filename) as f:
            for block in f.read().split(">")[1:]:
                head, _, seq = block.partition("\n")
                yield types.SimpleNamespace(id=head.split()[0], seq=seq.replace("\n", ""))
    bio.SeqIO.parse = parse
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, bio.SeqIO
    sys.path.insert(0, ref)
    import debruijn_graph as RG
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        flye = mp.write_flye_stub(tmp)
        for x, case in enumerate(mp.polish_cases()):
            outdir = os.path.join(tmp, "case_%d" % x, "polishing")
            scaffolds, pseudounits, rps, reads, monomers = mp.inputs(case)
            printed = io.StringIO()
            with contextlib.redirect_stdout(printed):
                RG.polish(scaffolds, pseudounits, rps, reads, monomers, outdir, case["n_iter"], case["n_threads"], flye_bin=flye)
            cases.append(dict(case, files=mp.tree_texts(outdir), printed=mp.printed_record(printed.getvalue(), outdir, flye)))
    files = [(c, fn, text) for c in cases for fn, text in c["files"].items()]
    reads_files = [(c, text) for c, fn, text in files if fn.endswith("reads.fasta")]
    assert any("'-'" in str(c["read_pseudounits"]) for c in cases) and any("'+'" in str(c["read_pseudounits"]) for c in cases)
    assert any(ch in text for _, text in reads_files for ch in "acgt") and any("N" in text.split("\n")[1] for _, text in reads_files)
    assert any(len(c["scaffolds"]) == 2 for c in cases)
    assert any(text.count(">") % 2 == 0 for _, text in reads_files)
    assert any(text.count(">") < sum(len(u) for s in c["read_pseudounits"] for u in s) for c, text in reads_files if len(c["scaffolds"]) == 1 and len(c["pseudounits"][0]) == 1), \
        "no duplicate segment id"
    by_dict_order = 0
    for c, fn, text in files:
        if fn.endswith("template.fasta"):
            recs = c["files"][fn.replace("template.fasta", "reads.fasta")].split("\n")
            ids, seqs = recs[0::2], recs[1::2]
            first = next(i for i, s in zip(ids, seqs) if len(s) == len(text.split("\n")[1]))
            by_dict_order += first != text.split("\n")[0]
    assert by_dict_order >= 1, "no template chosen by sorted order against dict order"
    with open(out_fn, "w") as f:
        json.dump({"source": "polish of scripts/debruijn_graph.py of the reference, captured by tools/capture_mono_polish_cases.py with a stub in Flye's place",
                   "cases": cases}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d files, %d bytes -> %s" % (len(cases), len(files), os.path.getsize(out_fn), out_fn))


if __name__ == "__main__":
    main()

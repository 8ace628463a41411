#!/usr/bin/env python3
"""Developer tool (BUILD CONTAINER ONLY: needs the reference checkout and pandas, no GPU): captures what the reference's
scripts/sd_parser.py makes of small String Decomposer reports into tests/golden/sd_parser_cases.json, the fixture that pins
centroflye_amd/sd_parser.py (tests/test_sd_parser.py).  The reference's module is imported as it is, with Bio.SeqIO.parse stubbed
by a few-line FASTA reader (as the tools/fuzz_*_vs_reference.py stub Biopython); nothing of it is copied.

Every case holds the report's text, the monomer FASTA's text, max_gap, and per read IN THE ORDER of SD_Report.monostrings the
string, the strand and mono2nucl (in its own order), the two name maps, and get_stats.  The hand-made cases come first: primed
monomers and reversed reads, a lower-case share of exactly 0.5, leading / trailing / inner '?', jumps of 100 and of 101 bases,
jumps whose ratio to the mean monomer length is exactly x.5, all-gap reads, interleaved read ids, 27 monomers; seeded random
cases follow.  Read ids are never all numeric (the reference's CSV reader would turn those into integers).
usage: tools/capture_sd_parser_cases.py [--reference DIR] [--random N] [--seed S]"""
import json
import os
import random
import sys
import tempfile
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sd_parser_cases.json")


def arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def fasta(lens, names=None):
    names = names or ["mon%d" % k for k in range(len(lens))]
    return "".join(">%s some description\n%s\n" % (n, "ACGT" * (x // 4) + "ACGT"[:x % 4]) for n, x in zip(names, lens)), names


def tsv(rows):
    return "".join("%s\t%s\t%d\t%d\t%.2f\t%s\n" % row for row in rows)


def chain(r_id, names, picks, start=0, length=10, jumps=None, rels=None, score=90.0):
    """rows of one read: instance x is monomer picks[x] (an index, or (index, True) for the primed one), `length` bases long, the
    jump st - previous en given by jumps[x] (1 unless said)"""
    rows, en = [], None
    for x, p in enumerate(picks):
        k, primed = p if isinstance(p, tuple) else (p, False)
        st = start if en is None else en + (jumps or {}).get(x, 1)
        en = st + length - 1
        rows.append((r_id, names[k] + ("'" if primed else ""), st, en, score, (rels or {}).get(x, "+")))
    return rows


def hand_made():
    cases = []
    f3, n3 = fasta([10, 12, 8])
    P = lambda k: (k, True)
    cases.append(("primed monomers, a reversed read next to a forward one", f3, 100,
                  chain("rd_rev", n3, [P(2), P(1), P(0), P(2)]) + chain("rd_fwd", n3, [0, 1, 2, 0])))
    cases.append(("a lower-case share of exactly 0.5 is not reversed; 3 of 5 is", f3, 100,
                  chain("half", n3, [0, P(1), 2, P(0)]) + chain("most", n3, [P(0), 1, P(2), P(1), 0])))
    cases.append(("leading, trailing and inner '?'", f3, 100,
                  chain("q_edges", n3, [0, 1, 2, 0, 1, 2, 0], rels={0: "?", 1: "?", 3: "?", 6: "?"}) +
                  chain("q_inner_rev", n3, [P(0), P(1), P(2), P(0)], rels={1: "?", 2: "-"})))
    cases.append(("jumps of 100 and of 101 bases at max_gap 100", f3, 100,
                  chain("j100", n3, [0, 1, 2], jumps={1: 100, 2: 101}) + chain("j101_rev", n3, [P(2), P(1), P(0)], jumps={1: 101, 2: 100})))
    f2, n2 = fasta([2, 2])
    cases.append(("jumps whose ratio to the mean monomer length 2 is x.5: 50.5 -> 50, 51.5 -> 52, 52.5 -> 52", f2, 100,
                  chain("half_even", n2, [0, 1, 0, 1], length=2, jumps={1: 101, 2: 103, 3: 105})))
    f4, n4 = fasta([3, 5])      # mean 4
    cases.append(("mean 4: 102 / 4 = 25.5 -> 26, 106 / 4 = 26.5 -> 26; max_gap 5: 6 / 4 = 1.5 -> 2, 10 / 4 = 2.5 -> 2", f4, 100,
                  chain("m4", n4, [0, 1, 0], length=4, jumps={1: 102, 2: 106})))
    cases.append(("the same monomers at max_gap 5", f4, 5,
                  chain("m4s", n4, [0, 1, 0, 1], length=4, jumps={1: 6, 2: 10, 3: 5})))
    cases.append(("all-gap reads give an empty string", f3, 100,
                  chain("all_q", n3, [0, 1, 2], rels={0: "?", 1: "?", 2: "?"}) + chain("one_q", n3, [1], rels={0: "?"}) +
                  chain("kept", n3, [0, 1])))
    a, b, c = chain("zz", n3, [0, 1, 2, 0]), chain("aa", n3, [P(2), P(1), P(0)]), chain("mm", n3, [1, 1])
    cases.append(("interleaved read ids come out grouped and sorted, rows in file order",
                  f3, 100, [a[0], b[0], c[0], a[1], a[2], b[1], c[1], b[2], a[3]]))
    f27, n27 = fasta([5 + k % 4 for k in range(27)], ["m%02d_x" % k for k in range(27)])
    cases.append(("27 monomers: the 27th has no letter, the mean is taken over all 27", f27, 100,
                  chain("r27", n27, [0, 25, P(25), 13, P(1)], length=6, jumps={2: 104, 4: 120}) +
                  chain("r27_rev", n27, [P(25), P(24), P(0)], length=6)))
    cases.append(("one read of one instance; gap symbols inside a reversed read next to a jump", f3, 100,
                  chain("single", n3, [1]) + chain("rev_gap", n3, [P(0), P(1), P(2), P(0), P(1)], jumps={2: 150, 4: 101}, rels={3: "?"})))
    return cases


def random_case(rng, c):
    K = rng.choice([1, 2, 3, 5, 12, 18, 26])
    lens = [rng.choice([2, 3, 7, 50, 170, 171]) for _ in range(K)]
    f, names = fasta(lens, ["%s%d" % (rng.choice(["mn", "A", "D6Z1_"]), k) for k in range(K)])
    max_gap = rng.choice([100, 100, 100, 5, 1000])
    reads = []
    for q in range(rng.randrange(1, 6)):
        r_id = "%s_%d%s" % (rng.choice(["read", "S1", "q"]), rng.randrange(1000), rng.choice(["", "/ccs", "x"]))
        p_prime = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        p_q = rng.choice([0.0, 0.1, 0.4, 1.0 if rng.random() < 0.1 else 0.2])
        n = rng.randrange(1, 14)
        picks = [(rng.randrange(K), rng.random() < p_prime) for _ in range(n)]
        jumps = {x: rng.choice([1, 1, 1, 0, 2, max_gap, max_gap + 1, max_gap + rng.randrange(2, 700)]) for x in range(1, n)}
        rels = {x: rng.choice(["?", "?", "-"]) for x in range(n) if rng.random() < p_q}
        reads.append(chain(r_id, names, picks, start=rng.randrange(0, 300), length=rng.choice([3, 150, 171]), jumps=jumps, rels=rels,
                           score=rng.choice([70.0, 88.24, 100.0])))
    ids = {rows[0][0] for rows in reads}
    if len(ids) < len(reads):
        reads = [rows for x, rows in enumerate(reads) if rows[0][0] not in {r[0][0] for r in reads[:x]}]
    rows = []
    if rng.random() < 0.4:      # interleave
        queues = [list(r) for r in reads]
        while any(queues):
            q = rng.choice([x for x in queues if x])
            rows.append(q.pop(0))
    else:
        rows = [row for r in reads for row in r]
    return ("random case %d" % c, f, max_gap, rows)


def main():
    ref = os.path.join(arg("--reference", "/root/reference"), "scripts")
    if not os.path.isdir(ref):
        sys.exit("this tool needs the reference checkout (--reference DIR; build container only)")
    sys.dont_write_bytecode = True

    def parse(filename, format=None):
        name, seq = None, []
        with open(filename) as f:
            for line in f:
                if line.startswith(">"):
                    if name is not None:
                        yield types.SimpleNamespace(id=name, seq="".join(seq))
                    name, seq = line[1:].split()[0], []
                else:
                    seq.append(line.strip())
        if name is not None:
            yield types.SimpleNamespace(id=name, seq="".join(seq))

    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")
    bio.SeqIO.parse = parse
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, bio.SeqIO
    sys.path.insert(0, ref)
    import sd_parser as RP
    rng = random.Random(arg("--seed", 27, int))
    cases = hand_made() + [random_case(rng, c) for c in range(arg("--random", 40, int))]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, fasta_text, max_gap, rows in cases:
            fa, rep = os.path.join(tmp, "monomers.fasta"), os.path.join(tmp, "decomposition.tsv")
            with open(fa, "w") as f:
                f.write(fasta_text)
            with open(rep, "w") as f:
                f.write(tsv(rows))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")      # (the mean of no letters of an all-gap read)
                report = RP.SD_Report(rep, fa, max_gap=max_gap)
                stats = RP.get_stats(report.monostrings)
            assert all(isinstance(k, str) for k in report.monostrings), name
            out.append(dict(
                name=name, tsv=tsv(rows), monomers_fasta=fasta_text, max_gap=max_gap,
                reads=[[r_id, ms.tostring(), ms.strand, [[int(c), m, int(st), int(en)] for c, (m, st, en) in ms.mono2nucl.items()]]
                       for r_id, ms in report.monostrings.items()],
                names_map=list(report.monomer_names_map.items()), rev_names_map=list(report.rev_monomer_names_map.items()),
                stats={k: (float(v) if k in ("mean_len", "pgaps") else int(v)) for k, v in stats.items()}))
    with open(OUT, "w") as f:
        json.dump(dict(source="scripts/sd_parser.py of the reference (SD_Report, get_stats), captured by tools/capture_sd_parser_cases.py",
                       cases=out), f, indent=0, sort_keys=True)
        f.write("\n")
    n_reads = sum(len(c["reads"]) for c in out)
    print("%d cases, %d reads, %d reversed, %d empty strings -> %s" % (
        len(out), n_reads, sum(r[2] == "-" for c in out for r in c["reads"]), sum(r[1] == "" for c in out for r in c["reads"]), OUT))


if __name__ == "__main__":
    main()

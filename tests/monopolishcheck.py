"""The inputs of tests/golden/mono_polish_cases.json and what turns a polish tree into a record: shared by
tools/capture_mono_polish_cases.py (which runs the reference's own ``polish`` on them, with a stub in Flye's place) and
tests/test_mono_polish.py (which runs centroflye_amd.debruijn_graph.polish and compares byte for byte); and the end-to-end input of
the cen6 driver's polishing stage (tests/test_emu_mono_polish_e2e.py, tests/test_gpu_mono_polish_e2e.py): a planted array of
nucleotides whose monomer instances carry their own substitutions, reads cut at monomer boundaries with noise applied per instance,
so that the decomposition rows can state the true boundaries."""
import os
import random
import stat

FLYE_STUB = '#!/bin/sh\n# FLYE --nano-raw READS --polish-target TEMPLATE -i N -t T -o DIR: the template as it is\ncp "$4" "${10}/polished_$6.fasta"\n'


def write_flye_stub(dirname):
    """a program in Flye's place that copies template.fasta to polished_N.fasta; its path"""
    fn = os.path.join(dirname, "flye_stub.sh")
    with open(fn, "w") as f:
        f.write(FLYE_STUB)
    os.chmod(fn, os.stat(fn).st_mode | stat.S_IXUSR)
    return fn


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def polish_cases(seed=35):
    """[case]: name, scaffolds, pseudounits, read_pseudounits as [[[key, st, en, strand] per read, in dict order] per unit] per
    scaffold (key = [id, part] or a plain id), reads, monomers, n_iter, n_threads"""
    rng = random.Random(seed)
    reads = {"r%d" % x: _seq(rng, 260) for x in range(12)}
    reads["low"] = _seq(rng, 200, "ACGTacgtNn-")
    reads["x"], reads["y"], reads["z"] = _seq(rng, 150), _seq(rng, 150, "ACGTacgtN"), _seq(rng, 150)
    monomers = {"m%d" % x: _seq(rng, 12) for x in range(5)}
    monomers.update({"m%d'" % x: "ACGT" for x in range(5)})
    P, M = "+", "-"

    def case(name, scaffolds, pseudounits, rps, n_iter=2, n_threads=3, ids=None):
        used = {(k[0] if isinstance(k, list) else k) for s in rps for u in s for k, _, _, _ in u} | set(ids or ())
        return dict(name=name, scaffolds=scaffolds, pseudounits=pseudounits, read_pseudounits=rps, reads={r: reads[r] for r in sorted(used)}, monomers=monomers,
                    n_iter=n_iter, n_threads=n_threads)

    return [
        case("three reads on the plus strand", ["ABCDE"], [[[0, 4]]], [[[[["r0", 0], 10, 69, P], [["r1", 0], 5, 66, P], [["r2", 0], 0, 62, P]]]]),
        case("three reads on the minus strand", ["ABCDE"], [[[0, 4]]], [[[[["r0", 0], 10, 69, M], [["r1", 0], 5, 66, M], [["r2", 0], 0, 62, M]]]]),
        case("both strands, lower case, N and '-' in a read", ["ABC"], [[[0, 2]]],
             [[[[["low", 0], 3, 90, M], [["low", 1], 100, 180, P], [["r3", 0], 20, 104, M], [["r4", 0], 0, 83, P], [["low", 2], 60, 150, M]]]]),
        case("(id, part) keys of cut reads: the parts of one read in one unit and in two", ["ABCABD"], [[[0, 2], [3, 5]]],
             [[[[["r5", 0], 0, 50, P], [["r5", 2], 120, 171, P], [["r6", 1], 30, 79, M]], [[["r5", 2], 172, 230, P], [["r6", 1], 80, 140, M], [["r7", 0], 9, 70, P]]]]),
        case("two scaffolds, the second with two units", ["ABCD", "EFGEF"], [[[0, 3]], [[0, 2], [3, 4]]],
             [[[[["r0", 0], 0, 80, P], [["r1", 0], 2, 84, M], [["r2", 0], 4, 83, P]]],
              [[[["r3", 0], 0, 40, M], [["r4", 0], 1, 43, P], [["r5", 0], 7, 46, P]], [[["r3", 0], 41, 100, M], [["r4", 0], 44, 101, P], [["r6", 0], 0, 58, M]]]]),
        case("an even number of reads: median_high takes the upper of the two middle lengths", ["AB"], [[[0, 1]]],
             [[[[["r0", 0], 0, 49, P], [["r1", 0], 0, 59, P], [["r2", 0], 0, 69, P], [["r3", 0], 0, 79, P]]]]),
        case("two reads only", ["AB"], [[[0, 1]]], [[[[["r8", 0], 0, 30, M], [["r9", 0], 0, 44, P]]]]),
        case("several reads of the median length: the first id in sorted order, not in dict order", ["ABC"], [[[0, 2]]],
             [[[[["r9", 0], 10, 59, P], [["r10", 0], 10, 59, M], [["r2", 0], 10, 59, P], [["r11", 0], 0, 70, P], [["r1", 0], 0, 20, P]]]]),
        case("sorted order is that of the segment ids as text: r10 before r2, _5_ before _50_", ["ABC"], [[[0, 2]]],
             [[[[["r2", 0], 50, 89, P], [["r2", 1], 5, 44, P], [["r10", 3], 100, 139, M]]]]),
        case("duplicate segment ids: two parts of one read with the same span, the later one overwrites in the earlier one's place", ["AB"], [[[0, 1]]],
             [[[[["r0", 0], 5, 64, P], [["r1", 0], 0, 70, P], [["r0", 1], 5, 64, M], [["r2", 0], 0, 50, P]]]]),
        case("one read: it is its own template", ["A"], [[[0, 0]]], [[[[["r7", 0], 11, 99, M]]]], n_iter=1, n_threads=50),
        case("plain one-character ids (the only plain keys the reference takes: r_id[0] is the id)", ["ABC"], [[[0, 2]]],
             [[[["x", 0, 70, P], ["y", 10, 85, M], ["z", 3, 80, P]]]], n_iter=3, n_threads=1),
    ]


def inputs(case):
    """the case as polish takes it: (scaffolds, pseudounits, read_pseudounits, reads, monomers)"""
    rps = [[{(tuple(k) if isinstance(k, list) else k): (st, en, strand) for k, st, en, strand in unit} for unit in s] for s in case["read_pseudounits"]]
    return case["scaffolds"], [[tuple(u) for u in s] for s in case["pseudounits"]], rps, case["reads"], case["monomers"]


def tree_texts(outdir):
    """{path relative to outdir: text} of every file below outdir"""
    out = {}
    for d, _, fs in os.walk(outdir):
        for fn in fs:
            with open(os.path.join(d, fn)) as f:
                out[os.path.relpath(os.path.join(d, fn), outdir).replace(os.sep, "/")] = f.read()
    return out


def printed_record(text, outdir, flye_bin):
    """the printed command lines with the two paths of the run replaced"""
    return text.replace(outdir, "OUTDIR").replace(flye_bin, "FLYE")


# ---------------------------------------------------------------- end to end: decomposition.tsv, monomers and reads -> polishing/
E2E = dict(seed=37, monomer_len=24, array_units=70, n_reads=24, read_units=25, inst_subs=0.03, p_del=0.02, p_sub=0.02, p_ins=0.015, k=40, min_mult=3, n_iter=2)
D6Z1 = "ABCDEFGHIJKLMNOPQR"
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_RC)[::-1]


def _noisy(rng, s, spec):
    out = []
    for x in s:
        u = rng.random()
        if u >= spec["p_del"]:
            out.append(rng.choice([c for c in "ACGT" if c != x]) if u < spec["p_del"] + spec["p_sub"] else x)
        if rng.random() < spec["p_ins"]:
            out.append(rng.choice("ACGT"))
    return "".join(out)


def e2e_inputs(spec=E2E):
    """(monomers.fasta, decomposition.tsv, reads.fasta, letters of the planted array, its instances as nucleotides): 18 random
    monomers; a planted array of the 18-letter HOR in which every unit carries another monomer at position 7 (no pair of
    neighbouring variants twice: every window of two units is unique) and every monomer INSTANCE its own substitutions; reads cut at
    monomer boundaries, the noise applied per instance so that the rows state the true boundaries; every third read on '-'; every
    eighth read starts at the array's first letter, the next one ends at its last."""
    rng = random.Random(spec["seed"])
    names = ["D6Z1_m%02d" % x for x in range(18)]
    monomers = [_seq(rng, spec["monomer_len"]) for _ in names]
    fasta = "".join(">%s\n%s\n" % (n, s) for n, s in zip(names, monomers))
    others = [c for c in D6Z1 if c != D6Z1[7]]
    pairs = [(a, b) for a in others for b in others]
    rng.shuffle(pairs)
    variants, seen = [rng.choice(others)], set()
    while len(variants) < spec["array_units"]:
        nxt = [b for a, b in pairs if a == variants[-1] and (a, b) not in seen]
        b = nxt[0] if nxt else rng.choice(others)
        seen.add((variants[-1], b))
        variants.append(b)
    letters = "".join(D6Z1[:7] + v + D6Z1[8:] for v in variants)
    instances = []
    for c in letters:
        s = list(monomers[ord(c) - 65])
        for x in range(len(s)):
            if rng.random() < spec["inst_subs"]:
                s[x] = rng.choice([b for b in "ACGT" if b != s[x]])
        instances.append("".join(s))
    rows, reads = [], []
    top = spec["array_units"] - spec["read_units"]
    for q in range(spec["n_reads"]):
        r_id = "read_%02d" % q
        start = 0 if q % 8 == 0 else 18 * top if q % 8 == 1 else 18 * rng.randrange(0, top) + rng.randrange(0, 18) * (q % 2)
        idx = list(range(start, min(start + 18 * spec["read_units"], len(letters))))
        noisy = [_noisy(rng, instances[x], spec) for x in idx]
        minus = q % 3 == 2
        if minus:
            idx, noisy = idx[::-1], [rc(s) for s in noisy[::-1]]
        at = 0
        for x, s in zip(idx, noisy):
            if s:
                rows.append("%s\t%s%s\t%d\t%d\t%.2f\t+\n" % (r_id, names[ord(letters[x]) - 65], "'" if minus else "", at, at + len(s) - 1, 92.5))
            at += len(s)
        reads.append(">%s\n%s\n" % (r_id, "".join(noisy)))
    return fasta, "".join(rows), "".join(reads), letters, instances


def write_e2e_inputs(tmp, spec=E2E):
    fasta, tsv, reads, letters, instances = e2e_inputs(spec)
    for name, text in (("monomers.fasta", fasta), ("decomposition.tsv", tsv), ("reads.fasta", reads)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    return letters, instances


def e2e_args(tmp, stop_after, spec=E2E):
    return ["--sd-report", os.path.join(tmp, "decomposition.tsv"), "--monomers", os.path.join(tmp, "monomers.fasta"), "--centromeric-reads",
            os.path.join(tmp, "reads.fasta"), "--outdir", os.path.join(tmp, "out_%s" % stop_after), "--min-k", str(spec["k"]), "--max-k", str(spec["k"]),
            "--min-mult", str(spec["min_mult"]), "--stop-after", stop_after, "--polisher", "consensus", "--polish-n-iter", str(spec["n_iter"])]


def scaffold_distances(engine, strings, truth):
    """the edit distance of every string to truth (cf_edit_distances, pinned by tests/editcheck.py)"""
    import numpy as np
    a_off = np.cumsum([0] + [len(x) for x in strings])
    # (pair p: a = strings[p], b = truth; cf_edit_distances takes one offset array per side, so truth is repeated per pair)
    data = "".join(strings) + truth * len(strings)
    b_off = a_off[-1] + len(truth) * np.arange(len(strings) + 1)
    return engine.edit_distances(data.encode(), a_off, b_off)[0].tolist()


def check_end_to_end(tmp, main, spec=E2E):
    """the driver's main with --stop-after polishing --polisher consensus on the generated inputs (the session's engine runs the
    kernels): the earlier stages' seven files and the polishing tree; every polished pseudounit and every TSV is the restatement on
    the exported files; the polished scaffold is nearer to the planted stretch than the joined templates; every base all of its
    three or more voting reads agree on is the planted base; and --stop-after pseudounits writes what it wrote and no polishing/"""
    import contextlib
    import io
    import conscheck as cc
    import monoscaffoldcheck as msc
    import supportcheck as sc
    tmp = str(tmp)
    letters, instances = write_e2e_inputs(tmp, spec)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert main(e2e_args(tmp, "polishing", spec)) == 0
    lines = printed.getvalue().splitlines()
    assert lines[-2:] == ["Reading centromeric reads", "Polishing"]
    out = os.path.join(tmp, "out_polishing")
    top = sorted(fn for fn in msc.listed(out) if not fn.startswith("polishing" + os.sep))
    assert top == sorted(msc.FILES)
    got = tree_texts(os.path.join(out, "polishing"))
    exported = {fn: text for fn, text in got.items() if fn.endswith(("/reads.fasta", "/template.fasta"))}
    want = sc.polish_tree_expected(exported, spec["n_iter"])
    assert set(got) == set(exported) | set(want)
    for fn in want:
        assert got[fn] == want[fn], fn
    with open(os.path.join(out, "scaffolds.tsv")) as f:
        scaffolds = [ln.rstrip("\n").split("\t")[2] for ln in f]
    with open(os.path.join(out, "pseudounits.tsv")) as f:
        units = [[int(x) for x in ln.split("\t")] for ln in f]
    assert len(scaffolds) == 1 and len(units) >= 20 and all(u[4] >= 1 for u in units)
    at = letters.find(scaffolds[0])
    assert at >= 0 and letters.find(scaffolds[0], at + 1) < 0      # the scaffold is one stretch of the planted array
    truth = "".join(instances[at:at + len(scaffolds[0])])
    polished = got["scaffold_0/scaffold_0.fasta"].split("\n")[1]
    templates = "".join(got[f"scaffold_0/pseudounit_{u[1]}/template.fasta"].split("\n")[1] for u in units)
    from centroflye_amd import session
    d_polished, d_templates = scaffold_distances(session.engine(), [polished, templates], truth)
    print("edit distance to the planted stretch of %d bases: joined templates %d, polished scaffold %d" % (len(truth), d_templates, d_polished))
    assert d_polished < d_templates
    support = [[int(x) for x in ln.split("\t")] for ln in got["scaffold_0/scaffold_0.support.tsv"].splitlines()]
    assert [s[0] for s in support] == list(range(len(polished)))
    checked = at_base = 0
    for _, j, st, en, _ in units:
        mine = [s for s in support if s[1] == j]
        unit = polished[at_base:at_base + len(mine)].encode()
        at_base += len(mine)
        planted = "".join(instances[at + st:at + en + 1]).encode()
        cols, _ = cc.walk(cc.matrix(unit, planted), unit, planted)
        for x, (_, _, agree, voting) in enumerate(mine):
            if agree == voting >= 3 and cols[x] is not None:
                assert cols[x] == unit[x], (j, x)
                checked += 1
    assert at_base == len(polished) and checked > len(polished) // 2
    # the stage before, on the same inputs: what it wrote, and no polishing directory
    with contextlib.redirect_stdout(io.StringIO()):
        assert main(e2e_args(tmp, "pseudounits", spec)) == 0
    before = os.path.join(tmp, "out_pseudounits")
    assert msc.listed(before) == sorted(msc.FILES) and not os.path.exists(os.path.join(before, "polishing"))
    for name in msc.FILES:
        with open(os.path.join(before, name)) as f1, open(os.path.join(out, name)) as f2:
            assert f1.read() == f2.read(), name
    return dict(units=len(units), bases=len(polished), d_templates=d_templates, d_polished=d_polished, checked=checked)

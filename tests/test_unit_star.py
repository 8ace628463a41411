"""Stage 4, the unit* reconstruction (scripts/better_consensus_unit_reconstruction.py), on CPU: the script on the emulated
kernels against the reference's goldens (tests/golden/make_golden_unit_star.py), cfh_unit_star on the random cases, the host HW
alignment against the reference's own edlib, the merge of the windows the device does not count, and the refusals."""
import hashlib
import heapq
import json
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import fixtures
from centroflye_amd import _host, session
from centroflye_amd import better_consensus_unit_reconstruction as B
from centroflye_amd.engine import Engine
from oracle import unit_kmers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRIPT = os.path.join(ROOT, "scripts", "better_consensus_unit_reconstruction.py")
LIBEDLIB = os.path.join(ROOT, "oracle", "_ref", "librr_ref.so")
NAMES = ("tiny", "lowcov", "hor2055", "exotic")


def edit_unit(unit, rot, subs):
    u = list(unit[rot:] + unit[:rot])
    for p, b in subs:
        u[p] = b
    return "".join(u)


def given_unit(report_path):
    pk = _host.parse_report(report_path, keep_rows=False)
    return pk.motifs[int(pk.meta[0][7])]


def top_digest(kmers, counts):
    return hashlib.sha256("".join(f"{x} {c}\n" for x, c in zip(kmers, counts)).encode()).hexdigest()


def expected_file(case):
    return f">unit*\n{case['unit_star']}\n".encode()


@pytest.fixture
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


@pytest.mark.parametrize("name", NAMES)
def test_script_writes_the_golden_bytes(emu_session, report, name, tmp_path):
    with open(os.path.join(GOLDEN, f"{name}.unit_star.json")) as f:
        g = json.load(f)
    rpt = report(name)
    assert fixtures.sha256_file(rpt) == g["report_sha256"]
    given = given_unit(rpt)
    for i, case in enumerate(g["cases"]):
        unit = edit_unit(given, case["rotation"], case["substitutions"])
        unit_fn = tmp_path / f"u{i}.fasta"
        unit_fn.write_text(f">unit\n{unit}\n")
        out = tmp_path / f"o{i}" / "cons_unit" / "unit_star.fasta"
        B.main(["--reads-ncrf", rpt, "--unit", str(unit_fn), "-k", str(case["k"]), "--output", str(out)])
        data = out.read_bytes()
        assert data == expected_file(case), (name, case["k"], case["rotation"])
        if case["hash_stable"]:
            assert hashlib.sha256(data).hexdigest() == case["main_sha256"]["1"]
        assert not os.path.exists(str(out) + ".tmp")
        # the top n the graph was built from
        pk = _host.parse_report(rpt, keep_rows=False)
        strs, cnts = B.top_kmers(pk, case["k"], case["n"])
        assert len(strs) == case["n_top"] and top_digest(strs, cnts) == case["top_digest"]


def _case_top(case):
    """Regenerate a random case's report and its top n by the numpy oracle (every window of every row)."""
    pk = _host.synth(pack=True, **case["synth"])
    rows = [pk.bases[pk.read_off[i]:pk.read_off[i + 1]].tobytes() for i in range(pk.n_reads)]
    keys, cnt = unit_kmers.kmer_occurrences(rows, case["k"])
    unit = edit_unit(pk.motifs[int(pk.meta[0][7])], case["rotation"], case["substitutions"])
    idx = unit_kmers.most_frequent(keys, cnt, B.n_top(unit, case["k"]))
    from centroflye_amd import kmers as km
    return km.decode(keys[idx], case["k"]) if idx.size else [], [int(c) for c in cnt[idx]], unit


def test_cfh_unit_star_on_the_random_cases():
    with open(os.path.join(GOLDEN, "unit_star_cases.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 40 and any("error" in c for c in cases) and not all(c["hash_stable"] for c in cases)
    for i, case in enumerate(cases):
        strs, cnts, unit = _case_top(case)
        assert len(strs) == case["n_top"] and top_digest(strs, cnts) == case["top_digest"], i
        if "error" in case:
            with pytest.raises(_host.UnitStarError) as ei:
                _host.unit_star(case["k"], strs, cnts, unit)
            assert ei.value.code in (-61, -62, -63, -64)
        else:
            assert _host.unit_star(case["k"], strs, cnts, unit)[0] == case["unit_star"], i


def test_graph_sizes_follow_the_reference():
    with open(os.path.join(GOLDEN, "hor2055.unit_star.json")) as f:
        g = json.load(f)
    pk = _host.synth(pack=True, **fixtures.FIXTURES["hor2055"]["synth"])
    for case in g["cases"]:
        unit = edit_unit(pk.motifs[int(pk.meta[0][7])], case["rotation"], case["substitutions"])
        rows = [pk.bases[pk.read_off[i]:pk.read_off[i + 1]].tobytes() for i in range(pk.n_reads)]
        keys, cnt = unit_kmers.kmer_occurrences(rows, case["k"])
        idx = unit_kmers.most_frequent(keys, cnt, case["n"])
        from centroflye_amd import kmers as km
        got, st = _host.unit_star(case["k"], km.decode(keys[idx], case["k"]), cnt[idx], unit)
        assert got == case["unit_star"]
        sizes = [[st["nodes_built"], st["edges_built"]], [st["nodes_collapsed"], st["edges_collapsed"]],
                 [st["nodes_tipped"], st["edges_tipped"]], [st["nodes_final"], st["edges_final"]]]
        assert sizes == case["graph_sizes"]


def _edlib():
    import ctypes as C
    if not os.path.exists(LIBEDLIB):
        pytest.skip("oracle/_ref/librr_ref.so (the reference's edlib) is not built here")

    class Cfg(C.Structure):
        _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int), ("eq", C.c_void_p), ("n_eq", C.c_int)]

    class Res(C.Structure):
        _fields_ = [("status", C.c_int), ("editDistance", C.c_int), ("endLocations", C.POINTER(C.c_int)),
                    ("startLocations", C.POINTER(C.c_int)), ("numLocations", C.c_int), ("alignment", C.c_void_p),
                    ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]

    lib = C.CDLL(LIBEDLIB)
    lib.edlibAlign.restype = Res
    lib.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, Cfg]
    lib.edlibFreeAlignResult.argtypes = [Res]

    def hw(q, t):
        r = lib.edlibAlign(q.encode(), len(q), t.encode(), len(t), Cfg(-1, 2, 1, None, 0))    # EDLIB_MODE_HW, EDLIB_TASK_LOC
        out = (r.editDistance, r.startLocations[0], r.endLocations[0])
        lib.edlibFreeAlignResult(r)
        return out
    return hw


def test_hw_alignment_matches_the_references_edlib():
    hw = _edlib()
    rng = random.Random(11)
    n = 0
    for _ in range(1500):
        m = rng.choice([1, 2, 5, 31, 63, 64, 65, 127, 128, 129, 300])
        alpha = rng.choice(["AC", "ACGT"])
        q = "".join(rng.choice(alpha) for _ in range(m))
        kind = rng.randrange(4)
        if kind == 0:       # a noisy doubled rotation: many equal end positions
            r = rng.randrange(m)
            t = "".join(c if rng.random() > 0.05 else rng.choice("ACGT") for c in (q[r:] + q[:r]) * 2)
        elif kind == 1:     # exact repeats: ties between copies
            t = q * rng.choice([1, 2, 3])
        elif kind == 2:     # short or unrelated targets (query longer than target, distance = query length)
            t = "".join(rng.choice("ACGTN") for _ in range(rng.choice([1, 3, 10, 70])))
        else:
            t = "".join(rng.choice(alpha) for _ in range(rng.choice([50, 200, 600])))
        assert _host.hw_locate(q, t) == hw(q, t), (q, t)
        n += 1
    # the stage's own shape: a DXZ1-sized unit against twice a rotated, edited copy
    u = "".join(rng.choice("ACGT") for _ in range(2055))
    v = list(u[700:] + u[:700])
    for p in rng.sample(range(2055), 9):
        v[p] = "A" if v[p] != "A" else "C"
    t = "".join(v) * 2
    assert _host.hw_locate(u, t) == hw(u, t)


def _n_everywhere(src, dst, motif):
    """A copy of the report whose rows hold an N in the middle of one 25-base stretch of the motif wherever it occurs (both
    orientations): k-mers over it are frequent enough to enter the top n."""
    rc = str.maketrans("ACGT", "TGCA")
    w = motif[40:65]
    pairs = [(w, w[:12] + "N" + w[13:])]
    pairs.append((w.translate(rc)[::-1], pairs[0][1].translate(rc)[::-1]))
    with open(src) as f:
        lines = f.read().split("\n")
    recs = [i for i, ln in enumerate(lines) if ln and not ln.startswith("#")][::2]
    for i in recs:
        head = lines[i].split(None, 4)
        row = head[4]
        for a, b in pairs:
            row = row.replace(a, b)
        lines[i] = " ".join(head[:4]) + " " + row
    with open(dst, "w") as f:
        f.write("\n".join(lines))


def test_windows_the_device_skips_are_merged_into_the_top_n(emu_session, report, tmp_path):
    k = 19
    src = report("tiny")
    motif = given_unit(src)
    rpt = str(tmp_path / "tiny_n.ncrf")
    _n_everywhere(src, rpt, motif)
    pk = _host.parse_report(rpt, keep_rows=False)
    assert pk.non_acgt
    # heapq.nlargest over every window of every row, as strings (the reference's get_most_frequent_kmers)
    counts = Counter()
    for i in range(pk.n_reads):
        row = pk.bases[pk.read_off[i]:pk.read_off[i + 1]].tobytes().decode()
        counts.update(row[j:j + k] for j in range(len(row) - k + 1))
    n = B.n_top(motif, k)
    want = heapq.nlargest(n, counts, key=lambda x: (counts[x], x))
    strs, cnts = B.top_kmers(pk, k, n)
    assert strs == want and cnts == [counts[x] for x in want]
    assert any("N" in x for x in strs), "the crafted input must put a window with an N into the top n"
    unit_fn = tmp_path / "u.fa"
    unit_fn.write_text(f">u\n{motif}\n")
    out = tmp_path / "out" / "unit_star.fasta"
    B.main(["--reads-ncrf", rpt, "--unit", str(unit_fn), "-k", str(k), "--output", str(out)])
    assert out.read_text() == f">unit*\n{_host.unit_star(k, want, [counts[x] for x in want], motif)[0]}\n"


def test_k_of_32_is_refused_and_leaves_no_file(report, tmp_path):
    unit_fn = tmp_path / "u.fasta"
    unit_fn.write_text(">u\nACGTACGTAC\n")
    out = tmp_path / "cons_unit" / "unit_star.fasta"
    r = subprocess.run([sys.executable, SCRIPT, "--reads-ncrf", report("tiny"), "--unit", str(unit_fn), "-k", "32",
                        "--output", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "k <= 31" in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")


def test_unit_fasta_follows_read_bio_seq(tmp_path):
    p = tmp_path / "u.fna"
    p.write_bytes(b"junk\n>first  some words\nAC gT\r\nnnA\t \n>second\nTTTT\n>first\nGGcc\n")
    assert B.read_unit(str(p)) == "GGcc"           # {id: seq}: the last record with the first id
    p = tmp_path / "u.fasta"
    p.write_bytes(b">a\nAC gT\r\nnnA \n>b\nTTTT\n")
    assert B.read_unit(str(p)) == "ACgTnnA"
    for ext in ("fq", "txt", "gz"):
        q = tmp_path / f"u.{ext}"
        q.write_text(">a\nACGT\n")
        with pytest.raises(ValueError, match="FASTA"):
            B.read_unit(str(q))


def test_reference_errors_are_refusals():
    # a lone 3-cycle: fine; a lone path: no edge survives the tips (the reference fails on edges[0])
    assert _host.unit_star(3, ["ACG", "CGA", "GAC"], [4, 4, 4], "ACG")[0] == "ACG"
    with pytest.raises(_host.UnitStarError) as ei:
        _host.unit_star(3, ["ACG", "CGT"], [4, 4], "ACGT")
    assert ei.value.code in (-61, -64)
    with pytest.raises(_host.UnitStarError) as ei:
        _host.unit_star(3, [], [], "ACGT")
    assert ei.value.code == -61

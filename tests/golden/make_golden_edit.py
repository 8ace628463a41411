#!/usr/bin/env python3
"""Golden vectors for the end of the polisher stage (scripts/eltr_polisher.py:116-157 read_polishing, compare_polished_sequences,
export_results; scripts/utils/bio.py:60-61 compress_homopolymer).  Build container only.

Distances: edlibAlign in mode NW of oracle/_ref/librr_ref.so (the reference's own vendored edlib, built by oracle/ref/Makefile),
through the stubs of make_golden_unit_star.py, on the seeded inputs of tests/editcheck.py.  Assembly: the reference's own
ELTR_Polisher methods by import, on trees fabricated by editcheck.fabricate_tree over the reference's own export of the `tiny`
and `lowcov` fixtures (one tree with multi-line FASTA, one with a gap position).

The script plants the misreadings editcheck.WRONG_RULES in editcheck's statements and fails unless each one changes a recorded
case.  (The clamp at n cannot change a DISTANCE — editcheck.fr says why — so that one has to show in the rows a run reaches.)

    python tests/golden/make_golden_edit.py            # writes edit_cases.json
    python tests/golden/make_golden_edit.py --check
"""
import hashlib
import json
import math
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import editcheck as ec  # noqa: E402
import fixtures  # noqa: E402
import make_golden_unit_star as U  # noqa: E402

SHAPE = dict(lane_bytes=32, turn_bytes=4096, lds_diags=16384)      # what cf_edit_info reports: the borders the inputs straddle


def import_reference():
    sys.dont_write_bytecode = True
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = U.bio_modules()
    sys.modules["edlib"] = U.edlib_module()
    if U.REF not in sys.path:
        sys.path.insert(0, U.REF)
    import eltr_polisher as E
    from utils.bio import compress_homopolymer
    return E, compress_homopolymer, sys.modules["edlib"]


def distance(edlib, a, b):
    if not a or not b:      # (the vendored edlib does not return for an empty string; the distance is the other one's length)
        return len(a) + len(b)
    return edlib.align(a.decode("latin-1"), b.decode("latin-1"))["editDistance"]


def tree_golden(E, spec, wd):
    report = fixtures.make_report(spec["fixture"], wd)
    csv = ec.placement_csv(spec["fixture"], wd)
    unit = os.path.join(wd, "unit.fasta")
    with open(unit, "w") as f:
        f.write(">u\nACGT\n")
    outdir = os.path.join(wd, spec["name"])
    params = types.SimpleNamespace(unit=unit, ncrf=report, outdir=outdir, read_placement=csv, min_pos=0, max_pos=math.inf,
                                   num_iters=spec["num_iters"])
    pol = E.ELTR_Polisher(params)
    files = pol.export_read_units(pol.map_pos2read())
    out = dict(spec, report_sha256=fixtures.sha256_file(report), inputs=ec.fabricate_tree(spec, outdir))
    if spec["gap"]:
        out["gap_position"] = ec.gap_position(outdir)
        del files[out["gap_position"]]
    try:
        finals = pol.read_polishing(files)
        pol.compare_polished_sequences(finals)
        pol.export_results(finals)
    except Exception as e:      # the reference raises: the drop-in must refuse
        out["error"] = type(e).__name__
        return out
    with open(os.path.join(outdir, "report.txt")) as f:
        out["report"] = f.read()
    out["files"] = {}
    for fn in sorted(os.listdir(outdir)):
        if fn.startswith("final_sequence"):
            with open(os.path.join(outdir, fn), "rb") as f:
                out["files"][fn] = hashlib.sha256(f.read()).hexdigest()
    out["final_lengths"] = [len(finals[i]) for i in range(1, spec["num_iters"] + 1)]
    return out


def build():
    E, compress, edlib = import_reference()
    g = dict(shape=SHAPE, single={}, offsets={}, trees={})
    singles = ec.single_cases(SHAPE["lane_bytes"], SHAPE["turn_bytes"]) + ec.switch_cases(SHAPE["lds_diags"]) + ec.big_cases()
    for name, a, b in singles:
        g["single"][name] = dict(sha_a=ec.sha(a), sha_b=ec.sha(b), n=len(a), m=len(b), distance=distance(edlib, a, b))
    for name, data, a_off, b_off, a, b in ec.offset_cases():
        g["offsets"][name] = dict(sha=ec.sha(data), distance=distance(edlib, a, b))
    data, a_off, b_off = ec.batch_case()
    g["batch"] = dict(sha=ec.sha(data), n_pairs=ec.BATCH_PAIRS,
                      distances=[distance(edlib, data[a_off[p]:a_off[p + 1]], data[b_off[p]:b_off[p + 1]]) for p in range(ec.BATCH_PAIRS)])
    for long_runs in (True, False):
        data, off, seqs = ec.hpc_case(long_runs)
        want = [compress(s.decode()).encode() for s in seqs]
        g["hpc_long" if long_runs else "hpc_short"] = dict(sha_in=ec.sha(data), sha_out=ec.sha(b"".join(want)), lengths=[len(s) for s in want])
    with tempfile.TemporaryDirectory() as wd:
        for spec in ec.TREES:
            g["trees"][spec["name"]] = tree_golden(E, spec, wd)

    # the planted misreadings: each has to change a recorded case
    small = [(name, a, b) for name, a, b in singles if len(a) * len(b) <= 250000]
    kills = {r: 0 for r in ec.WRONG_RULES}
    for name, a, b in small:
        want = g["single"][name]["distance"]
        assert ec.nw(a, b) == want and ec.fr(a, b) == want, name
        kills["n_matches_anything"] += ec.nw(a, b, "n_matches_anything") != want
        kills["case_folding"] += ec.nw(a, b, "case_folding") != want
        d, reach = ec.fr(a, b, wrong="no_clamp_at_n", want_reach=True)
        assert d == want, name      # (never the distance)
        kills["no_clamp_at_n"] += reach > len(a)
        assert ec.fr(a, b, want_reach=True)[1] <= len(a)
    data, off, seqs = ec.hpc_case(True)
    got = b"".join(ec.hpc(s) for s in seqs)
    assert ec.sha(got) == g["hpc_long"]["sha_out"]
    # (a tile border of the device scan inside a run: the statement on the whole buffer with the borders of sequences kept)
    kills["hpc_resets_at_tile_borders"] += any(ec.hpc(s, "hpc_resets_at_tile_borders") != ec.hpc(s) for s in seqs)
    g["wrong_rule_kills"] = {r: int(v) for r, v in kills.items()}
    missing = [r for r, v in kills.items() if not v]
    if missing:
        sys.exit(f"no recorded case tells {missing} from the reference")
    return g


def main():
    g = json.loads(json.dumps(build()))
    path = ec.GOLDEN
    if "--check" in sys.argv:
        with open(path) as f:
            same = json.load(f) == g
        print(os.path.basename(path), "IDENTICAL" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(path, "w") as f:
        json.dump(g, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes", g["wrong_rule_kills"])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the unit extractor and the unit clusterer (scripts/unit_extractor.py:23-136, scripts/unit_clusterer.py:29-78).
Runs the reference itself by import (build container only): its get_repetitive_kmers, get_convolution, get_period_info,
get_hook_kmer, split_by_hook, select_median_seq and its own write_bio_seqs on the seeded inputs of tests/tandemcheck.py, in the
order run_on_read and unit_clusterer.main call them (Flye and the plot are left out).  Biopython is the FASTA reader stub of
make_golden_unit_star.py; matplotlib is the real one.

Recorded per read: the counts, the head and the digest of periods / bin_convs, bin_left / bin_right, the hook and its tandem index,
the split ids (number and digest), med_len, the template, the SHA-256 of both files.  The script fails unless tandemcheck's numpy
statement gives the same on every case and every misreading of tandemcheck.WRONG_RULES changes at least one recorded case.

    python tests/golden/make_golden_tandem.py            # writes tests/golden/tandem_cases.json
"""
import json
import os
import statistics
import sys
import tempfile
from bisect import bisect_left, bisect_right

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/scripts"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import tandemcheck as tc  # noqa: E402
from make_golden_unit_star import bio_modules  # noqa: E402


def import_reference():
    sys.dont_write_bytecode = True
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio_modules()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import unit_clusterer as UC
    import unit_extractor as UE
    from utils.bio import write_bio_seqs
    return UE, UC, write_bio_seqs


def file_sha(write, seqs, tmp):
    fn = os.path.join(tmp, "x.fasta")
    write(fn, seqs)
    with open(fn, "rb") as f:
        return tc.sha(f.read())


def record_read(UE, write, seq, k, bin_size, tmp):
    s = seq.decode("latin-1")
    rep = UE.get_repetitive_kmers(s, k)
    conv, union = UE.get_convolution(rep)
    rec = dict(n_rep_kmers=len(rep), n_conv=len(union), period=None)
    if not union:      # run_on_read raises on periods[0]
        return rec
    periods, bin_convs, bin_left, bin_right = UE.get_period_info(union, bin_size=bin_size)
    hook = UE.get_hook_kmer(conv, bin_left, bin_right)
    assert hook is not None
    splits = UE.split_by_hook(s, hook)
    med_len = statistics.median_high([len(x) for x in splits.values()])
    template = next(r_id for r_id in sorted(splits.keys()) if len(splits[r_id]) == med_len)
    # the windows the loop visits: one per pass of its `while r < len(conv)`
    n_windows = 1 + next(l for l in range(len(union)) if union[-1] - union[l] <= 2 * bin_size)
    rec.update(period=periods[0], count=bin_convs[0], bin_left=bin_left, bin_right=bin_right, n_windows=n_windows,
               periods_head=list(periods[:8]), bin_convs_head=list(bin_convs[:8]), n_periods=len(periods),
               tuples_sha=tc.sha(json.dumps([list(periods), list(bin_convs)]).encode()),
               hook=hook, hook_index=bisect_right(conv[hook], bin_right) - bisect_left(conv[hook], bin_left),
               n_splits=len(splits), split_ids_sha=tc.sha("\n".join(splits.keys()).encode()), med_len=med_len, template=template,
               splits_sha=file_sha(write, splits, tmp), median_sha=file_sha(write, {template: splits[template]}, tmp))
    return rec


def record_cluster(UE, UC, write, bin_size, units, tmp):
    lens = sorted(len(u) for u in units.values())
    periods, bin_convs, bin_left, bin_right = UE.get_period_info(lens, bin_size=bin_size)
    filt = {k: v for k, v in units.items() if bin_left <= len(v) <= bin_right}
    rec = dict(sha_in=tc.sha(json.dumps(units, sort_keys=True).encode()), periods=list(periods), bin_convs=list(bin_convs), bin_left=bin_left,
               bin_right=bin_right, cluster_ids=list(filt))
    try:
        median_id, median_unit, median_len = UC.select_median_seq(filt)
    except UnboundLocalError:      # no unit has statistics.median's length
        rec["raises"] = True
        return rec
    rec.update(raises=False, median_id=median_id, median_len=median_len, cluster_sha=file_sha(write, filt, tmp),
               median_sha=file_sha(write, {median_id: median_unit}, tmp))
    return rec


def main():
    UE, UC, write = import_reference()
    out = dict(shape=tc.SHAPE, cases={}, clusters={}, wrong_rule_kills={})
    all_cases = tc.cases()
    with tempfile.TemporaryDirectory() as tmp:
        for case in all_cases:
            data, _ = tc.pack(case["reads"])
            out["cases"][case["name"]] = dict(k=case["k"], bin_size=case["bin_size"], sha_in=tc.sha(data), ids=case["ids"],
                                              reads=[record_read(UE, write, s, case["k"], case["bin_size"], tmp) for s in case["reads"]])
        for name, bin_size, units in tc.cluster_cases():
            out["clusters"][name] = record_cluster(UE, UC, write, bin_size, units, tmp)
    # the numpy statement agrees everywhere; every misreading is told apart somewhere
    facts = dict(even_best=0, odd_best=0, period_differs_from_best_l=0, hor_period_off=0)
    for case in all_cases:
        recs = out["cases"][case["name"]]["reads"]
        for i, (seq, res, rec) in enumerate(zip(case["reads"], tc.restate_case(case), recs)):
            got = tc.summary(seq, res, case["k"])
            assert not tc.differs(rec, got) and rec.get("n_windows") == got.get("n_windows"), (case["name"], i, rec, got)
            if rec["period"] is not None:
                facts["even_best" if rec["count"] % 2 == 0 else "odd_best"] += 1
        for seq, res, rec in zip(case["reads"], tc.restate_case(case, "period_of_best_l"), recs):
            facts["period_differs_from_best_l"] += rec["period"] is not None and res["period"] != rec["period"]
        if case["name"] == "hor64":
            assert len(recs) == 64
            facts["hor_period_off"] = max(abs(r["period"] - 2055) for r in recs)
            assert facts["hor_period_off"] <= case["bin_size"]
    assert facts["even_best"] and facts["odd_best"] and facts["period_differs_from_best_l"], facts
    for wrong in tc.WRONG_RULES:
        kills = 0
        for case in all_cases:
            for seq, res, rec in zip(case["reads"], tc.restate_case(case, wrong), out["cases"][case["name"]]["reads"]):
                kills += tc.differs(rec, tc.summary(seq, res, case["k"]))
        assert kills >= 1, f"no recorded case tells '{wrong}' from the reference"
        out["wrong_rule_kills"][wrong] = kills
    out["facts"] = facts
    path = os.path.join(HERE, "tandem_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(path) < 250_000, os.path.getsize(path)
    print(path, os.path.getsize(path), out["wrong_rule_kills"], facts)


if __name__ == "__main__":
    main()

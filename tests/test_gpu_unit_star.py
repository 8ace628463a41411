"""Stage 4, the unit* reconstruction, on the MI355X: the script on the fixtures and the random cases against the reference's
goldens (tests/golden/make_golden_unit_star.py), and at the bench's size (50 000 synthetic reads) the device top n against
oracle/unit_kmers.py's selection and the unit* against the generator's own motif."""
import json
import os

import numpy as np
import pytest

import fixtures
from centroflye_amd import _host, session
from centroflye_amd import better_consensus_unit_reconstruction as B
from centroflye_amd import kmers as km
from oracle import unit_kmers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def edit_unit(unit, rot, subs):
    u = list(unit[rot:] + unit[:rot])
    for p, b in subs:
        u[p] = b
    return "".join(u)


def run_script(tmp_path, tag, report, unit, k):
    unit_fn = tmp_path / f"{tag}.fasta"
    unit_fn.write_text(f">unit\n{unit}\n")
    out = tmp_path / tag / "cons_unit" / "unit_star.fasta"
    B.main(["--reads-ncrf", str(report), "--unit", str(unit_fn), "-k", str(k), "--output", str(out)])
    return out.read_bytes()


@pytest.fixture
def gpu_session():
    session.reset()
    yield session
    session.reset()


def test_fixtures_and_random_cases_through_the_script(gpu_session, report, tmp_path):
    for name in ("tiny", "lowcov", "hor2055", "exotic"):
        with open(os.path.join(GOLDEN, f"{name}.unit_star.json")) as f:
            g = json.load(f)
        rpt = report(name)
        assert fixtures.sha256_file(rpt) == g["report_sha256"]
        pk = _host.parse_report(rpt, keep_rows=False)
        given = pk.motifs[int(pk.meta[0][7])]
        for i, case in enumerate(g["cases"]):
            data = run_script(tmp_path, f"{name}{i}", rpt, edit_unit(given, case["rotation"], case["substitutions"]), case["k"])
            assert data == f">unit*\n{case['unit_star']}\n".encode(), (name, i)
    with open(os.path.join(GOLDEN, "unit_star_cases.json")) as f:
        cases = json.load(f)["cases"]
    for i, case in enumerate(cases):
        rpt = tmp_path / f"case{i}.ncrf"
        _host.synth(report_path=str(rpt), pack=False, **case["synth"])
        pk = _host.parse_report(str(rpt), keep_rows=False)
        unit = edit_unit(pk.motifs[int(pk.meta[0][7])], case["rotation"], case["substitutions"])
        if "error" in case:
            with pytest.raises(SystemExit) as ei:
                run_script(tmp_path, f"c{i}", rpt, unit, case["k"])
            assert ei.value.code not in (0, None)
            assert not (tmp_path / f"c{i}" / "cons_unit" / "unit_star.fasta").exists()
        else:
            assert run_script(tmp_path, f"c{i}", rpt, unit, case["k"]) == f">unit*\n{case['unit_star']}\n".encode(), i


def test_bench_size_top_n_and_unit_star(gpu_session, tmp_path):
    """50 000 reads of the bench's workload; --unit = the generator's motif rotated by 37 with three substitutions."""
    import bench
    k = 30
    rpt = tmp_path / "bench50k.ncrf"
    _host.synth(report_path=str(rpt), pack=False, n_reads=50000, **bench.synth_kwargs(50000, 2))
    pk = _host.parse_report(str(rpt), keep_rows=False)
    motif = pk.motifs[int(pk.meta[0][7])]
    rot, subs = 37, [[100, "A" if motif[137] != "A" else "C"], [1000, "G" if motif[1037] != "G" else "T"],
                     [2000, "C" if motif[(2037) % len(motif)] != "C" else "A"]]
    unit = edit_unit(motif, rot, subs)
    n = B.n_top(unit, k)
    strs, cnts = B.top_kmers(pk, k, n)
    # the device's top n against the oracle's selection rule over the device's whole occurrence table (the rule ranks by (count,
    # k-mer), so every member has a count >= the n-th largest: it runs on those entries; the table needs no host-side sort)
    e = session.engine()
    keys, lo, hi = e.table(sort=False)
    cnt = lo.astype(np.int64) | (hi.astype(np.int64) << 32)
    thr = np.partition(cnt, cnt.size - n)[cnt.size - n] if cnt.size > n else 0
    cand = np.flatnonzero(cnt >= thr)
    want = cand[unit_kmers.most_frequent(keys[cand], cnt[cand], n)]
    assert strs == km.decode(keys[want], k) and cnts == [int(c) for c in cnt[want]]
    assert int(cnt.sum()) == sum(max(0, int(pk.read_off[i + 1] - pk.read_off[i]) - k + 1) for i in range(pk.n_reads))
    (tmp_path / "u.fasta").write_text(f">unit\n{unit}\n")
    got, st = B.run(B.parse_args(["--reads-ncrf", str(rpt), "--unit", str(tmp_path / "u.fasta"), "-k", str(k),
                                  "--output", str(tmp_path / "out" / "unit_star.fasta")]))
    assert got == _host.unit_star(k, strs, cnts, unit)[0]
    assert got == motif[rot:] + motif[:rot], f"unit* is not the motif in the given unit's phase: graph {st}"

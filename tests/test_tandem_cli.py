"""scripts/unit_extractor.py and scripts/unit_clusterer.py end to end (the extractor's batch on the host-emulated kernels) against the
REFERENCE's recorded files (tests/golden/tandem_cases.json: SHA-256 of what its own write_bio_seqs wrote): splits.fasta and
median_read_unit.fasta per read, periods.tsv, reads without a period, 8-character id collisions and --full-ids, a duplicate id, the
reference's Flye argv, the clusterer's files, its failure exits with nothing written, and the chain extractor -> clusterer."""
import json
import os
import runpy
import stat
import sys

import pytest

import tandemcheck as tc
from centroflye_amd import session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = tc.load_cases()
CASES = {c["name"]: c for c in tc.cases()}


def run_script(name, argv, emu_lib=None):
    """(exit code, stdout + stderr is left to capsys)."""
    session.reset()
    if emu_lib is not None:
        session._engine = Engine(0, emu_lib)
    old = sys.argv
    try:
        sys.argv = [name] + [str(a) for a in argv]
        runpy.run_path(os.path.join(ROOT, "scripts", name), run_name="__main__")
        return 0
    except SystemExit as e:
        return 0 if e.code is None else e.code
    finally:
        sys.argv = old
        session.reset()


def write_fasta(path, ids, reads, width=0):
    with open(path, "wb") as f:
        for i, s in zip(ids, reads):
            f.write(b">" + i.encode() + b" some description\n")
            if width:
                for o in range(0, len(s), width):
                    f.write(s[o:o + width] + b"\n")
            else:
                f.write(s + b"\n")


def check_tree(out, ids, recs, name_of=lambda i: i[:8]):
    for i, rec in zip(ids, recs):
        d = out / name_of(i)
        if rec["period"] is None:
            assert not d.exists(), i
            continue
        assert sorted(os.listdir(d)) == ["median_read_unit.fasta", "splits.fasta"], i
        assert tc.sha((d / "splits.fasta").read_bytes()) == rec["splits_sha"], i
        assert tc.sha((d / "median_read_unit.fasta").read_bytes()) == rec["median_sha"], i


@pytest.mark.parametrize("name", ["noisy_k6_bin3", "exotic", "lengths_around_k", "bin_size_0"])
def test_the_extractor_writes_the_reference_s_files(emu_lib, tmp_path, name):
    case, g = CASES[name], G["cases"][name]
    fa = tmp_path / "reads.fasta"
    write_fasta(fa, case["ids"], case["reads"], width=60 if name == "exotic" else 0)
    out = tmp_path / "out"
    assert run_script("unit_extractor.py", ["-i", fa, "-o", out, "-k", case["k"], "-b", case["bin_size"]], emu_lib) == 0
    check_tree(out, case["ids"], g["reads"])
    lines = (out / "periods.tsv").read_text().splitlines()
    assert lines[0].startswith("#id\tstatus\tlength") and len(lines) == len(case["ids"]) + 2
    periods = []
    for ln, i, seq, rec in zip(lines[1:], case["ids"], case["reads"], g["reads"]):
        f = ln.split("\t")
        assert len(f) == 14 and f[0] == i and int(f[2]) == len(seq) and (int(f[3]), int(f[4])) == (rec["n_rep_kmers"], rec["n_conv"])
        if rec["period"] is None:
            assert f[1] == "no_period" and f[5:] == [".", ".", ".", ".", ".", "0", "0", ".", "."]
        else:
            periods.append(rec["period"])
            assert f[1] == "ok" and f[5:] == [str(rec[c]) for c in ("period", "bin_left", "bin_right", "count", "hook", "hook_index")] + \
                [str(rec["n_splits"]), str(rec["med_len"]), rec["template"]]
    import statistics
    assert lines[-1] == f"# median period of {len(periods)} reads: {statistics.median(periods)}"


def test_fastq_gz_input_and_no_reads(emu_lib, tmp_path):
    import gzip
    case, g = CASES["perfect_tandem"], G["cases"]["perfect_tandem"]
    fq = tmp_path / "reads.fq.gz"
    with gzip.open(fq, "wb") as f:
        for i, s in zip(case["ids"], case["reads"]):
            f.write(b"@" + i.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    out = tmp_path / "out"
    assert run_script("unit_extractor.py", ["-i", fq, "-o", out], emu_lib) == 0
    check_tree(out, case["ids"], g["reads"])
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b"")
    assert run_script("unit_extractor.py", ["-i", empty, "-o", tmp_path / "out2"], emu_lib) == 0
    assert (tmp_path / "out2" / "periods.tsv").read_text().splitlines()[-1] == "# median period of 0 reads: ."


def test_ids_that_share_eight_characters_and_full_ids(emu_lib, tmp_path, capsys):
    case, g = CASES["perfect_tandem"], G["cases"]["perfect_tandem"]
    ids = ["m54329_180_a", "m54329_180_b"]
    fa = tmp_path / "reads.fasta"
    write_fasta(fa, ids, case["reads"])
    out = tmp_path / "out"
    assert run_script("unit_extractor.py", ["-i", fa, "-o", out], emu_lib) == 0
    err = capsys.readouterr().err
    assert "m54329_180_a" in err and "m54329_180_b" in err and "later one wins" in err
    assert sorted(os.listdir(out)) == ["m54329_1", "periods.tsv"]
    assert tc.sha((out / "m54329_1" / "splits.fasta").read_bytes()) == g["reads"][1]["splits_sha"]      # the later read, as in the reference
    out = tmp_path / "full"
    assert run_script("unit_extractor.py", ["-i", fa, "-o", out, "--full-ids"], emu_lib) == 0
    assert "later one wins" not in capsys.readouterr().err
    check_tree(out, ids, g["reads"], name_of=lambda i: i)


def test_a_duplicate_id_exits_before_anything_is_written(emu_lib, tmp_path, capsys):
    case = CASES["perfect_tandem"]
    fa = tmp_path / "reads.fasta"
    write_fasta(fa, ["same", "same"], case["reads"])
    assert run_script("unit_extractor.py", ["-i", fa, "-o", tmp_path / "out"], emu_lib) == 1
    assert "occurs twice" in capsys.readouterr().err and not (tmp_path / "out").exists()
    assert run_script("unit_extractor.py", ["-i", fa, "-o", tmp_path / "out", "-k", 32], emu_lib) == 2
    assert not (tmp_path / "out").exists()


def test_polish_runs_the_reference_s_flye_command_per_read(emu_lib, tmp_path):
    case = CASES["perfect_tandem"]
    fa = tmp_path / "reads.fasta"
    write_fasta(fa, case["ids"], case["reads"])
    log = tmp_path / "argv.jsonl"
    flye = tmp_path / "flye"
    flye.write_text(f"#!{sys.executable}\nimport json, sys\nopen({str(log)!r}, 'a').write(json.dumps(sys.argv[1:]) + '\\n')\n")
    flye.chmod(flye.stat().st_mode | stat.S_IXUSR)
    out = tmp_path / "out"
    assert run_script("unit_extractor.py", ["-i", fa, "-o", out, "--polish", "--flye-bin", flye], emu_lib) == 0
    calls = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert calls == [["--nano-raw", str(out / i / "splits.fasta"), "--polish-target", str(out / i / "median_read_unit.fasta"), "-i", "2", "-t", "50",
                      "-o", str(out / i)] for i in case["ids"]]


# ---------------------------------------------------------------------------------------------- the clusterer
def cluster_inputs():
    return {name: (bin_size, units) for name, bin_size, units in tc.cluster_cases()}


@pytest.mark.parametrize("name", sorted(G["clusters"]))
def test_the_clusterer_against_the_reference(tmp_path, capsys, name):
    bin_size, units = cluster_inputs()[name]
    g = G["clusters"][name]
    assert tc.sha(json.dumps(units, sort_keys=True).encode()) == g["sha_in"]
    src, out = tmp_path / "units", tmp_path / "out"
    for d, u in units.items():
        os.makedirs(src / d)
        (src / d / "polished_2.fasta").write_text(f">contig_1\n{u[:70]}\n{u[70:]}\n")
    (src / "a_file_not_a_directory.txt").write_text("x")
    rc = run_script("unit_clusterer.py", ["-i", src, "-o", out, "-b", bin_size])
    if g["raises"]:
        assert rc == 1 and "falls between two lengths" in capsys.readouterr().err and not out.exists()
        return
    assert rc == 0 and sorted(os.listdir(out)) == ["cluster_units.fasta", "median_read_unit.fasta"]
    assert tc.sha((out / "cluster_units.fasta").read_bytes()) == g["cluster_sha"]
    assert tc.sha((out / "median_read_unit.fasta").read_bytes()) == g["median_sha"]
    assert (out / "median_read_unit.fasta").read_text().split("\n")[0] == ">" + g["median_id"]


def test_the_clusterer_s_failures_write_nothing(tmp_path, capsys):
    out = tmp_path / "out"
    assert run_script("unit_clusterer.py", ["-i", tmp_path / "missing", "-o", out]) == 1
    assert "is not a directory" in capsys.readouterr().err and not out.exists()
    empty = tmp_path / "empty"
    empty.mkdir()
    assert run_script("unit_clusterer.py", ["-i", empty, "-o", out]) == 1
    assert "holds no directory" in capsys.readouterr().err and not out.exists()
    (empty / "read1").mkdir()
    assert run_script("unit_clusterer.py", ["-i", empty, "-o", out]) == 1
    assert "polished_2.fasta is missing" in capsys.readouterr().err and not out.exists()


def test_the_chain_extractor_to_clusterer(emu_lib, tmp_path):
    case, g = CASES["noisy_k6_bin3"], G["cases"]["noisy_k6_bin3"]
    fa = tmp_path / "reads.fasta"
    write_fasta(fa, case["ids"], case["reads"])
    units, out = tmp_path / "units", tmp_path / "cluster"
    assert run_script("unit_extractor.py", ["-i", fa, "-o", units, "-k", case["k"], "-b", case["bin_size"]], emu_lib) == 0
    rc = run_script("unit_clusterer.py", ["-i", units, "-o", out, "-b", 3, "--units-name", "median_read_unit.fasta"])
    # the same choice from the recorded med_len of every read, by the rules of unit_clusterer.py:64-78 in numpy terms
    import numpy as np
    import statistics
    lens = {i: rec["med_len"] for i, rec in zip(case["ids"], g["reads"]) if rec["period"] is not None}
    conv = np.sort(list(lens.values()))
    cnt = np.searchsorted(conv, conv + 6, "right") - np.arange(conv.size)
    l = int(np.argmax(cnt))
    bl, br = conv[l], conv[l + cnt[l] - 1]
    cluster = sorted(i for i, n in lens.items() if bl <= n <= br)
    med = statistics.median([lens[i] for i in cluster])
    want = next((i for i in cluster if lens[i] == med), None)
    if want is None:
        assert rc == 1 and not out.exists()
        return
    assert rc == 0
    heads = [ln[1:] for ln in (out / "cluster_units.fasta").read_text().splitlines() if ln.startswith(">")]
    assert heads == cluster
    assert (out / "median_read_unit.fasta").read_text() == f">{want}\n" + (units / want / "median_read_unit.fasta").read_text().split("\n")[1] + "\n"

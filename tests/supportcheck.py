"""The support rule and the per-read rule of the consensus polisher (include/cfhip.h at cf_consensus_run; cf_consensus_support,
cf_consensus_reads) restated in plain Python on top of conscheck.matrices and conscheck.walk, the hand-written cases that pin the
restatement, and the bodies shared by tests/test_emu_support.py and tests/test_gpu_support.py.

The rule: every byte a pass emits carries one number, `agree`:
* an inserted base at (slot s, k): the largest of its four tallies — the tally of the base emitted;
* a column base: 0 if all five tallies are 0 (the template byte kept with no vote; c_v == 0 is such a case), else the tally of the
  base emitted, which after the tie rule is the top tally;
* a column resolved as "deleted" emits nothing and has no entry.
Per read: `voted`, and `dist` = its distance to the pass's template if it voted, -1 if it did not (the band stopped at the permille
limit, or the lengths alone put the read beyond it: the distance was never established).

``LITERALS`` have the expected `agree` written out; ``WRONG_RULES`` are misreadings of the support rule, each an option of
``one_pass``; ``killers`` says which literal tells each from the rule."""
import numpy as np

import conscheck as cc

K_INS = cc.K_INS
BASES = cc.BASES
WRONG_RULES = ("support_is_c_v", "support_is_the_templates_tally", "support_counts_excluded", "support_of_iteration_1")


# ---------------------------------------------------------------- the rule
def one_pass(t, reads, permille=300, wrong=None):
    """(output, agree of every output byte, voting reads, excluded reads, [dist of every read], [voted of every read])."""
    t = bytes(t)
    m = len(t)
    # [0]: the tallies of the voting reads, which decide the bytes; [1]: those of every read (a misreading's support only)
    col = [[[0] * 5 for _ in range(m)] for _ in range(2)]
    ins = [[[[0] * 4 for _ in range(K_INS)] for _ in range(m + 1)] for _ in range(2)]
    c_v, dist, voted = 0, [], []
    for r, D in zip(reads, cc.matrices(t, reads)):
        r = bytes(r)
        d = int(D[m][len(r)])
        votes = 1000 * d <= permille * m
        voted.append(votes)
        dist.append(d if votes else -1)
        c_v += votes
        cols, runs = cc.walk(D, t, r)
        for w in ((0, 1) if votes else (1,)):
            for i, x in enumerate(cols):
                if x is None:
                    col[w][i][4] += 1
                elif x in BASES:
                    col[w][i][BASES.index(x)] += 1
            for s, run in runs.items():
                for k, x in enumerate(run[:K_INS]):
                    if x in BASES:
                        ins[w][s][k][BASES.index(x)] += 1
    sup = 1 if wrong == "support_counts_excluded" else 0
    out, agree = bytearray(), []
    for s in range(m + 1):
        for k in range(K_INS):
            if not 2 * sum(ins[0][s][k]) > c_v:
                break
            win = ins[0][s][k].index(max(ins[0][s][k]))
            out.append(BASES[win])
            agree.append(ins[sup][s][k][win])
        if s < m:
            top = max(col[0][s])
            if top == 0:
                out.append(t[s])
                agree.append(0)
                continue
            tied = [x for x in range(5) if col[0][s][x] == top]
            win = tied[0]
            if t[s] in BASES and BASES.index(t[s]) in tied:
                win = BASES.index(t[s])
            if win < 4:
                out.append(BASES[win])
                if wrong == "support_is_the_templates_tally":
                    agree.append(col[0][s][BASES.index(t[s])] if t[s] in BASES else 0)
                else:
                    agree.append(col[sup][s][win])
    if wrong == "support_is_c_v":
        agree = [c_v] * len(out)
    return bytes(out), agree, c_v, len(reads) - c_v, dist, voted


def consensus(t, reads, n_iters=1, permille=300, wrong=None):
    """[(output, agree, voting, excluded, dist, voted) of iteration 1 .. n_iters]."""
    res = []
    for _ in range(n_iters):
        res.append(one_pass(t, reads, permille, wrong))
        t = res[-1][0]
    if wrong == "support_of_iteration_1":
        res = [r[:1] + (res[0][1],) + r[2:] for r in res]
    return res


# ---------------------------------------------------------------- literal cases
# (name, template, reads, permille, [(output, agree) per iteration], [(dist, voted as 0 / 1) per iteration] or None)
LITERALS = (
    ("unanimous_column", b"ACGT", [b"ACGT", b"ACGT", b"ACGT"], 1000, [(b"ACGT", [3, 3, 3, 3])], [([0, 0, 0], [1, 1, 1])]),
    ("substitution_2_to_1", b"ACGT", [b"AGGT", b"AGGT", b"ACGT"], 1000, [(b"AGGT", [3, 2, 3, 3]), (b"AGGT", [3, 2, 3, 3])],
     [([1, 1, 0], [1, 1, 1]), ([0, 0, 1], [1, 1, 1])]),
    ("tie_kept_by_the_template", b"ACGT", [b"AGGT", b"ACGT"], 1000, [(b"ACGT", [2, 1, 2, 2])], None),
    ("tie_without_the_templates_base", b"ATGT", [b"ACGT", b"AGGT"], 1000, [(b"ACGT", [2, 1, 2, 2])], None),
    ("majority_deletion_has_no_entry", b"TACGA", [b"ACG", b"ACG", b"TACGA"], 1000, [(b"ACG", [3, 3, 3])], [([2, 2, 0], [1, 1, 1])]),
    ("inserted_run_of_1", b"ACT", [b"ACGT", b"ACGT", b"ACT"], 1000, [(b"ACGT", [3, 3, 2, 3])], None),
    ("inserted_run_of_4", b"AATT", [b"AACGCGTT", b"AACGCGTT", b"AATT"], 2000, [(b"AACGCGTT", [3, 3, 2, 2, 2, 2, 3, 3])], None),
    ("inserted_run_of_5", b"AATT", [b"AACGCGCTT", b"AACGCGCTT"], 2000, [(b"AACGCGTT", [2] * 8), (b"AACGCGCTT", [2] * 9)], [([5, 5], [1, 1]), ([1, 1], [1, 1])]),
    ("insertion_at_exactly_half", b"ACT", [b"ACGT", b"ACT"], 1000, [(b"ACT", [2, 2, 2])], None),
    ("read_N_on_a_column", b"ACGT", [b"ANGT", b"ANGT"], 1000, [(b"ACGT", [2, 0, 2, 2])], [([1, 1], [1, 1])]),
    ("read_N_against_one_vote", b"ACGT", [b"ANGT", b"ANGT", b"ACGT"], 1000, [(b"ACGT", [3, 1, 3, 3])], None),
    ("no_voting_read", b"ACGT", [b"TTTTTTTT"], 300, [(b"ACGT", [0, 0, 0, 0]), (b"ACGT", [0, 0, 0, 0])], [([-1], [0]), ([-1], [0])]),
    # 200 permille of 10 bytes: d = 2 votes (1000 d == P m), d = 3 does not
    ("read_at_the_limit_and_one_edit_beyond", b"ACGTACGTAC", [b"ACTTAAGTAC", b"ACTTAAGTGC", b"ACTTAAGTGC"], 200,
     [(b"ACTTAAGTAC", [1] * 10), (b"ACTTAAGTGC", [3, 3, 3, 3, 3, 3, 3, 3, 2, 3])],      # (all three are within the limit of iteration 1's output)
     [([2, -1, -1], [1, 0, 0]), ([0, 1, 1], [1, 1, 1])]),
    ("excluded_reads_do_not_count", b"ACGTACGTAC", [b"ACGTAGCGTAC", b"ACGTAGCGTAC", b"TTTTTTTTTT", b"TTTTTTTTTT"], 200, [(b"ACGTAGCGTAC", [2] * 11)],
     [([1, 1, -1, -1], [1, 1, 0, 0])]),
    ("empty_template_with_reads", b"", [b"ACG", b""], 300, [(b"", [])], [([-1, 0], [0, 1])]),
    ("position_with_no_reads", b"ACGT", [], 300, [(b"ACGT", [0, 0, 0, 0])], [([], [])]),
)


def check_literals_pin_the_restatement():
    for name, t, reads, permille, want, per_read in LITERALS:
        got = consensus(t, reads, len(want), permille)
        assert [(g[0], g[1]) for g in got] == [(w[0], list(w[1])) for w in want], name
        if per_read is not None:
            assert [(g[4], [int(v) for v in g[5]]) for g in got] == [(list(d), list(v)) for d, v in per_read], name
        # the bytes and the counts are conscheck's
        assert [(g[0], g[2], g[3]) for g in got] == cc.consensus(t, reads, len(want), permille), name


def killers():
    """{misreading: [literal cases on which it gives another agree than the rule]}."""
    res = {w: [] for w in WRONG_RULES}
    for name, t, reads, permille, want, _ in LITERALS:
        for w in WRONG_RULES:
            got = consensus(t, reads, len(want), permille, w)
            assert [g[0] for g in got] == [x[0] for x in want], (name, w)      # a misreading of the support leaves the bytes alone
            if [g[1] for g in got] != [list(x[1]) for x in want]:
                res[w].append(name)
    return res


# ---------------------------------------------------------------- device and restatement side by side
_expected = {}


def expected(positions, n_iters=1, permille=300):
    """[[(output, agree, voting, excluded, dist, voted) per position] per iteration] from the restatement; computed once per input."""
    key = (tuple((bytes(t), tuple(bytes(r) for r in rs)) for t, rs in positions), n_iters, permille)
    if key not in _expected:
        per_pos = [consensus(t, rs, n_iters, permille) for t, rs in positions]
        _expected[key] = [[per_pos[p][i] for p in range(len(positions))] for i in range(n_iters)]
    return _expected[key]


def device(engine, positions, n_iters=1, permille=300):
    """The same from one cf_consensus_run, cf_consensus_get, cf_consensus_support and cf_consensus_reads of every iteration."""
    t, t_off, r, r_off, pos_ptr = cc.pack(positions)
    res = engine.consensus_run(t, t_off, r, r_off, pos_ptr, n_iters=n_iters, permille=permille, support=True)
    out = []
    for i, (b, off, nv, ne) in enumerate(res, 1):
        agree = engine.consensus_support(i)
        dist, voted = engine.consensus_reads(i)
        assert agree.dtype == np.int32 and agree.shape == (b.size,) and off[-1] == b.size, i
        assert dist.dtype == np.int32 and voted.dtype == np.bool_ and dist.shape == voted.shape == (int(pos_ptr[-1]),), i
        for p in range(len(positions)):
            a = agree[off[p]:off[p + 1]]
            assert a.size == 0 or (0 <= int(a.min()) and int(a.max()) <= int(nv[p])), (i, p)
        out.append([(b[off[p]:off[p + 1]].tobytes(), agree[off[p]:off[p + 1]].tolist(), int(nv[p]), int(ne[p]), dist[pos_ptr[p]:pos_ptr[p + 1]].tolist(),
                     voted[pos_ptr[p]:pos_ptr[p + 1]].tolist()) for p in range(len(positions))])
    return out


def check(engine, positions, n_iters=2, permille=300):
    """device == restatement, field by field, and cf_consensus_get's outputs are conscheck.expected's: nothing moved."""
    got, want = device(engine, positions, n_iters, permille), expected(positions, n_iters, permille)
    old = cc.expected(positions, n_iters, permille)
    for i in range(n_iters):
        for p in range(len(positions)):
            what = f"iteration {i + 1}, position index {p} (template of {len(positions[p][0])} bytes, {len(positions[p][1])} reads)"
            assert (got[i][p][0], got[i][p][2], got[i][p][3]) == old[i][p], what
            for f, name in enumerate(("output", "agree", "voting", "excluded", "dist", "voted")):
                assert got[i][p][f] == want[i][p][f], what + ": " + name
    return got


def check_literals(engine):
    """Every literal case as a call of its own against the written-out figures, and all of one permille as one call."""
    for name, t, reads, permille, want, per_read in LITERALS:
        got = device(engine, [(t, reads)], len(want), permille)
        assert [(g[0][0], g[0][1]) for g in got] == [(w[0], list(w[1])) for w in want], name
        if per_read is not None:
            assert [(g[0][4], [int(v) for v in g[0][5]]) for g in got] == [(list(d), list(v)) for d, v in per_read], name
    for permille in sorted({c[3] for c in LITERALS}):
        cases = [c for c in LITERALS if c[3] == permille]
        got = device(engine, [(c[1], c[2]) for c in cases], 1, permille)
        assert [(g[0], g[1]) for g in got[0]] == [(c[4][0][0], list(c[4][0][1])) for c in cases], permille


def length_positions(lengths=(1, 2, 3, 4, 5, 63, 64, 65), seed=20261601):
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        t = cc.rand_seq(rng, m)
        out.append((t, [cc.noisy(rng, t, 0.06, 0.06, 0.06) for _ in range(4)] + [t, cc.rand_seq(rng, m + 2)]))
    return out


def slot_count_positions(slots, seed=20261602):
    """Several positions whose global slots (bytes + one per position) add up to `slots`: the last thread of the vote block's
    grid-stride loop and the K_INS + 1 entries per thread of the compaction meet a block edge."""
    rng = np.random.default_rng(seed + slots)
    lengths = [61, 0, 97, 33]
    lengths.append(slots - sum(lengths) - len(lengths) - 1)
    out = []
    for m in lengths:
        t = cc.rand_seq(rng, m)
        out.append((t, [cc.noisy(rng, t, 0.05, 0.05, 0.08) for _ in range(3)]))
    assert sum(len(t) for t, _ in out) + len(out) == slots
    return out


def random_positions(n=200, seed=20261603):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t, reads, _ = cc.position(rng, int(rng.integers(1, 97)), int(rng.integers(0, 10)), p_del=0.05, p_sub=0.05, p_ins=0.05)
        out.append((t[:96], reads))
    return out


def check_iterations_keep_their_own_support(engine):
    """Two and three iterations of positions whose output grows from pass to pass: support of iteration k is that of iteration k's votes."""
    positions = [(b"AATT", [b"AACGCGCTT", b"AACGCGCTT"]), (b"AATT", [b"AACGCGCGCGCTT", b"AACGCGCGCGCTT", b"AACGCGCGCGCTT"])]
    for n_iters in (2, 3):
        got = check(engine, positions, n_iters, 4000)
        assert len(got[0][0][1]) < len(got[1][0][1]) and len(got[0][1][1]) < len(got[1][1][1])      # more entries in the second pass
        for i in range(1, n_iters + 1):      # asked for again out of order
            assert engine.consensus_support(i).tolist() == [a for g in got[i - 1] for a in g[1]]


def check_batches(engine):
    rng = np.random.default_rng(20261604)
    t, reads, _ = cc.position(rng, 60, 9, p_del=0.04, p_sub=0.04, p_ins=0.04)
    positions = [(t, reads), (cc.rand_seq(rng, 50), [b"T" * 50, b"G" * 47]), cc.many_reads_positions((4,), 60)[0]]
    want = check(engine, positions, 2)
    before = engine.consensus_info()["n_batches"]
    for batch_bytes in (700, 1):
        with engine.knobs(cons_batch_bytes=batch_bytes):
            assert check(engine, positions, 2) == want
            assert engine.consensus_info()["n_batches"] > before


def check_more_positions_than_the_launch_cap(engine):
    positions = cc.many_positions(engine.consensus_info()["launch_cap"] + 3)
    check(engine, positions, 1)
    info = engine.consensus_info()
    assert info["n_reads"] > info["launch_cap"]


def check_refusals(engine):
    """Iteration 0 and n_iters + 1 are refused with -22 by both entry points, NULL outputs are taken, and the last run stays intact."""
    lib, ctx = engine._lib, engine._ctx
    good = [(b"ACGTACGTAC", [b"ACGTAGCGTAC", b"ACGTAGCGTAC", b"ACGTACGTAC", b"TTTTTTTTTT"])]
    want = check(engine, good, 2, 300)
    for it in (0, 3, -1):
        assert lib.cf_consensus_support(ctx, it, None) == -22
        assert b"cf_consensus_support" in lib.cf_last_error(ctx)
        assert lib.cf_consensus_reads(ctx, it, None, None) == -22
        assert b"cf_consensus_reads" in lib.cf_last_error(ctx)
    assert lib.cf_consensus_support(None, 1, None) == -22 and lib.cf_consensus_reads(None, 1, None, None) == -22
    for it in (1, 2):
        assert lib.cf_consensus_support(ctx, it, None) == 0 and lib.cf_consensus_reads(ctx, it, None, None) == 0
        dist = np.full(4, 77, np.int32)
        assert lib.cf_consensus_reads(ctx, it, dist.ctypes.data, None) == 0 and dist.tolist() == want[it - 1][0][4]
        voted = np.full(4, 77, np.uint8)
        assert lib.cf_consensus_reads(ctx, it, None, voted.ctypes.data) == 0 and voted.astype(bool).tolist() == want[it - 1][0][5]
        assert engine.consensus_support(it).tolist() == want[it - 1][0][1]
    # a refused run leaves the support of the run before
    import pytest
    from centroflye_amd.engine import DeviceError
    with pytest.raises(DeviceError):
        device(engine, good, 0)
    assert engine.consensus_support(2).tolist() == want[1][0][1] and engine.consensus_reads(1)[0].tolist() == want[0][0][4]
    with pytest.raises(DeviceError):
        engine.consensus_support(3)
    with pytest.raises(DeviceError):
        engine.consensus_reads(0)
    # a run without support (cf_consensus_run) gives the same bytes and leaves nothing to ask for
    assert cc.device(engine, good, 2) == [[(g[0], g[2], g[3]) for g in per_pos] for per_pos in want]
    for it in (1, 2):
        assert lib.cf_consensus_support(ctx, it, None) == -22 and b"with support" in lib.cf_last_error(ctx)
        assert lib.cf_consensus_reads(ctx, it, None, None) == -22 and b"with support" in lib.cf_last_error(ctx)
        assert lib.cf_consensus_get(ctx, it, None, None, None, None) == 0
    assert check(engine, good, 2, 300) == want


# ---------------------------------------------------------------- the tree of debruijn_graph.polish(polisher='consensus')
def _records(text):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1 and all(ln.startswith(">") for ln in lines[0:-1:2]), "two lines per record"
    return [(h[1:], s) for h, s in zip(lines[0:-1:2], lines[1:-1:2])]


def polish_tree_expected(files, n_iter, permille=300):
    """{path: text} that polisher='consensus' has to write beside the exported reads.fasta and template.fasta of `files` ({path
    relative to the polishing directory: text}): every polished_k.fasta, the scaffolds, consensus_report.tsv, read_votes.tsv and the
    support files, from the restatement on the exported strings (letters a .. z upper-cased for the run).  A unit without reads
    passes as it is and is flagged."""
    units = sorted((int(fn.split("/")[0][9:]), int(fn.split("/")[1][11:])) for fn in files if fn.endswith("/template.fasta"))
    want = {}
    report = ["scaffold\tunit\treads\ttemplate\ttemplate_length" + "".join(f"\tlength_{k}\tvoting_{k}\texcluded_{k}" for k in range(1, n_iter + 1)) + "\tuncovered\n"]
    votes, support, scaffolds = [], {}, {}
    for i, j in units:
        d = f"scaffold_{i}/pseudounit_{j}"
        (t_id, t), = _records(files[d + "/template.fasta"])
        reads = _records(files[d + "/reads.fasta"])
        res = expected([(t.encode().upper(), [r.encode().upper() for _, r in reads])], n_iter, permille)
        row = f"{i}\t{j}\t{len(reads)}\t{t_id}\t{len(t)}"
        for k, per_pos in enumerate(res, 1):
            out, agree, nv, ne, dist, voted = per_pos[0]
            want[d + f"/polished_{k}.fasta"] = f">consensus_s_{i}_t_{j}_iter_{k}\n{out.decode()}\n"
            row += f"\t{len(out)}\t{nv}\t{ne}"
        report.append(row + f"\t{int(not reads)}\n")
        for q, (r_id, _) in enumerate(reads):
            votes.append(f"{i}\t{j}\t{r_id}" + "".join(f"\t{per_pos[0][4][q]}\t{int(per_pos[0][5][q])}" for per_pos in res) + "\n")
        scaffolds[i] = scaffolds.get(i, "") + out.decode()
        lines = support.setdefault(i, [])
        for a in agree:
            lines.append(f"{len(lines)}\t{j}\t{a}\t{nv}\n")
    want["consensus_report.tsv"] = "".join(report)
    want["read_votes.tsv"] = "".join(votes)
    for i in scaffolds:
        want[f"scaffold_{i}/scaffold_{i}.fasta"] = f">scaffold_{i}_niter_{n_iter}\n{scaffolds[i]}\n"
        want[f"scaffold_{i}/scaffold_{i}.support.tsv"] = "".join(support[i])
    return want

"""The rule of the built-in consensus polisher (cf_consensus.hip; include/cfhip.h at cf_consensus_run) restated in plain Python, the
cases that pin the restatement, and the bodies shared by tests/test_emu_consensus.py and tests/test_gpu_consensus.py.

There is no reference function behind the polisher: the rule is the specification.  So

* ``LITERALS`` are hand-written cases with the expected bytes written out: they pin ``consensus`` itself;
* ``WRONG_RULES`` are plausible misreadings of the rule, each an option of the same functions; ``killers`` says which committed
  case tells each one from the rule — without one the cases could not tell a wrong kernel from a right one;
* everything else compares the device with ``consensus`` byte for byte.

``matrix`` is the full unit-cost NW matrix (a numpy row at a time; ``matrices`` the same for several reads at once), ``walk`` the walk back from (m, n) with the preference
(a) diagonal, (b) deletion, (c) insertion, ``one_pass`` the exclusion, the votes and the emission.
"""
import numpy as np

K_INS = 4
WRONG_RULES = ("prefers_b_over_a", "right_aligns_runs", "column_ties_by_order", "insertion_at_half", "counts_excluded")
BASES = b"ACGT"


# ---------------------------------------------------------------- the rule
def matrix(t, r):
    """D[i][j] = edit distance of t[:i] and r[:j]: (m + 1) x (n + 1)."""
    a = np.frombuffer(bytes(t), np.uint8)
    b = np.frombuffer(bytes(r), np.uint8)
    dt = np.int16 if max(a.size, b.size) < 16000 else np.int32
    D = np.empty((a.size + 1, b.size + 1), dt)
    j = np.arange(b.size + 1, dtype=np.int32)
    D[0] = j
    prev = j.copy()
    cur = np.empty_like(prev)
    for i in range(a.size):
        # min(deletion, diagonal), then the insertions along the row: D[i][j] - j is a running minimum
        cur[0] = i + 1
        np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i]), out=cur[1:])
        cur -= j
        np.minimum.accumulate(cur, out=prev)
        prev += j
        D[i + 1] = prev
    return D


def matrices(t, reads, group=8):
    """matrix(t, r) of every read, yielded in order; the rows of `group` reads are computed together (a cell with j <= n depends on
    no column beyond n, so the padding behind a shorter read changes nothing)."""
    a = np.frombuffer(bytes(t), np.uint8)
    group = max(1, min(group, 10 ** 8 // max(1, a.size * max([len(r) for r in reads] + [1]))))      # (D of a group: 200 MB at most)
    for g in range(0, len(reads), group):
        rs = [np.frombuffer(bytes(r), np.uint8) for r in reads[g:g + group]]
        width = max(r.size for r in rs)
        if len(rs) == 1 or a.size * width < 4096:
            for r in rs:
                yield matrix(t, r)
            continue
        b = np.zeros((len(rs), width), np.uint8)
        for q, r in enumerate(rs):
            b[q, :r.size] = r
        dt = np.int16 if max(a.size, width) < 16000 else np.int32
        D = np.empty((len(rs), a.size + 1, width + 1), dt)
        j = np.arange(width + 1, dtype=dt)
        D[:, 0] = j
        cur = np.empty((len(rs), width + 1), dt)
        for i in range(a.size):
            prev = D[:, i]
            cur[:, 0] = i + 1
            np.add(prev[:, :-1], b != a[i], out=cur[:, 1:], dtype=dt)
            np.minimum(cur[:, 1:], prev[:, 1:] + dt(1), out=cur[:, 1:])
            cur -= j
            np.minimum.accumulate(cur, axis=1, out=D[:, i + 1])
            D[:, i + 1] += j
        for q, r in enumerate(rs):
            yield D[q, :, :r.size + 1]


def walk(D, t, r, wrong=None):
    """(columns, runs): columns[i] = the read byte on column i or None when the column is deleted in this read; runs[s] = the
    bytes inserted in slot s, in read order."""
    m, n = len(t), len(r)
    cols, runs = [None] * m, {}
    i, j = m, n
    while i > 0 or j > 0:
        here = int(D[i, j])
        a = i > 0 and j > 0 and int(D[i - 1, j - 1]) + (t[i - 1] != r[j - 1]) == here
        b = i > 0 and int(D[i - 1, j]) + 1 == here
        if wrong == "prefers_b_over_a" and b:
            a = False
        if a:
            cols[i - 1] = r[j - 1]
            i, j = i - 1, j - 1
        elif b:
            i -= 1
        else:
            runs[i] = bytes([r[j - 1]]) + runs.get(i, b"")
            j -= 1
    return cols, runs


def one_pass(t, reads, permille=300, wrong=None):
    """(output, voting reads, excluded reads, [d of every read])."""
    t = bytes(t)
    m = len(t)
    col = [[0] * 5 for _ in range(m)]
    ins = [[[0] * 4 for _ in range(K_INS)] for _ in range(m + 1)]
    c_v, dists = 0, []
    for r, D in zip(reads, matrices(t, reads)):
        r = bytes(r)
        d = int(D[m][len(r)])
        dists.append(d)
        if 1000 * d > permille * m:
            continue
        c_v += 1
        cols, runs = walk(D, t, r, wrong)
        for i, x in enumerate(cols):
            if x is None:
                col[i][4] += 1
            elif x in BASES:
                col[i][BASES.index(x)] += 1
        for s, run in runs.items():
            if wrong == "right_aligns_runs":
                run = run[-K_INS:]
                run = bytes(K_INS - len(run)) + run      # (a zero byte casts no vote)
            for k, x in enumerate(run[:K_INS]):
                if x in BASES:
                    ins[s][k][BASES.index(x)] += 1
    n_voting = c_v
    if wrong == "counts_excluded":
        c_v = len(reads)
    out = bytearray()
    for s in range(m + 1):
        for k in range(K_INS):
            v = sum(ins[s][k])
            if not (2 * v >= c_v and v > 0 if wrong == "insertion_at_half" else 2 * v > c_v):
                break
            out.append(BASES[ins[s][k].index(max(ins[s][k]))])
        if s < m:
            top = max(col[s])
            if top == 0:
                out.append(t[s])
                continue
            tied = [x for x in range(5) if col[s][x] == top]
            win = tied[0]
            if wrong != "column_ties_by_order" and t[s] in BASES and BASES.index(t[s]) in tied:
                win = BASES.index(t[s])
            if win < 4:
                out.append(BASES[win])
    return bytes(out), n_voting, len(reads) - n_voting, dists


def consensus(t, reads, n_iters=1, permille=300, wrong=None):
    """[(output, voting, excluded) of iteration 1 .. n_iters]: iteration i has the output of i - 1 as its template."""
    res = []
    for _ in range(n_iters):
        t, nv, ne, _ = one_pass(t, reads, permille, wrong)
        res.append((t, nv, ne))
    return res


# ---------------------------------------------------------------- literal cases: (name, template, reads, permille, [expected output per iteration])
# (the tiny ones run at 1000 or 2000 permille: at the default 300 a 3- or 4-byte template takes no read with an edit)
LITERALS = (
    ("majority_substitution", b"ACGT", [b"AGGT", b"AGGT", b"ACGT"], 1000, [b"AGGT"]),
    ("tie_kept_by_the_template", b"ACGT", [b"AGGT", b"ACGT"], 1000, [b"ACGT"]),
    ("tie_kept_by_the_template_against_the_order", b"AGGT", [b"ACGT", b"AGGT"], 1000, [b"AGGT"]),
    ("tie_without_the_templates_base", b"ATGT", [b"ACGT", b"AGGT"], 1000, [b"ACGT"]),
    ("insertion_at_exactly_half", b"ACT", [b"ACGT", b"ACT"], 1000, [b"ACT"]),
    ("insertion_above_half", b"ACT", [b"ACGT", b"ACGT", b"ACT"], 1000, [b"ACGT"]),
    ("insertions_at_slot_0_and_slot_m", b"CCGG", [b"ACCGGT", b"ACCGGT", b"CCGG"], 1000, [b"ACCGGT"]),
    ("inserted_run_of_5", b"AATT", [b"AACGCGCTT", b"AACGCGCTT"], 2000, [b"AACGCGTT", b"AACGCGCTT", b"AACGCGCTT"]),
    ("deleted_first_and_last_column", b"TACGA", [b"ACG", b"ACG", b"TACGA"], 1000, [b"ACG"]),
    ("read_N_casts_no_vote", b"ACGT", [b"ANGT", b"ANGT", b"ACGT"], 1000, [b"ACGT"]),
    ("template_N_without_votes_is_kept", b"ANGT", [b"ANGT", b"ANGT"], 1000, [b"ANGT"]),
    ("no_voting_read", b"ACGT", [b"TTTTTTTT"], 300, [b"ACGT", b"ACGT"]),
    ("empty_template", b"", [b"ACG", b""], 300, [b""]),
    ("empty_read_excluded", b"ACG", [b""], 300, [b"ACG"]),
    ("empty_reads_delete_everything", b"ACG", [b"", b""], 1000, [b""]),
    ("both_between_a_and_b", b"AAT", [b"AT", b"AT", b"AGT", b"AGT"], 1000, [b"AAT"]),
    # 200 permille of 10 bytes: d = 2 votes (1000 d == P m), d = 3 does not
    ("read_at_the_limit_and_one_edit_beyond", b"ACGTACGTAC", [b"ACTTAAGTAC", b"ACTTAAGTGC", b"ACTTAAGTGC"], 200, [b"ACTTAAGTAC"]),
    ("excluded_reads_do_not_count", b"ACGTACGTAC", [b"ACGTAGCGTAC", b"ACGTAGCGTAC", b"TTTTTTTTTT", b"TTTTTTTTTT"], 200, [b"ACGTAGCGTAC"]),
)
LITERAL_COUNTS = {"read_at_the_limit_and_one_edit_beyond": (1, 2), "excluded_reads_do_not_count": (2, 2), "no_voting_read": (0, 1),
                  "empty_template": (1, 1), "empty_read_excluded": (0, 1)}


def killers():
    """{misreading: [literal cases on which it gives other bytes than the rule]}."""
    res = {w: [] for w in WRONG_RULES}
    for name, t, reads, permille, want in LITERALS:
        for w in WRONG_RULES:
            if [x[0] for x in consensus(t, reads, len(want), permille, w)] != list(want):
                res[w].append(name)
    return res


# ---------------------------------------------------------------- seeded inputs
def rand_seq(rng, n, alphabet=BASES):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def noisy(rng, s, p_del=0.02, p_sub=0.02, p_ins=0.015):
    """A read of s at the generator's error rates: every base deleted, substituted, followed by an inserted base."""
    out = bytearray()
    for x in s:
        u = rng.random()
        if u < p_del:
            pass
        elif u < p_del + p_sub:
            out.append(BASES[(BASES.index(x) + 1 + int(rng.integers(0, 3))) % 4] if x in BASES else x)
        else:
            out.append(x)
        if rng.random() < p_ins:
            out.append(BASES[int(rng.integers(0, 4))])
    return bytes(out)


def position(rng, length, n_reads, **rates):
    """(template, reads, truth): the template is a noisy copy of the unit like the reads (the median read unit is a read)."""
    truth = rand_seq(rng, length)
    return noisy(rng, truth, **rates)[:max(length, 1) * 2], [noisy(rng, truth, **rates) for _ in range(n_reads)], truth


def delete_bytes(rng, s, d):
    keep = np.ones(len(s), bool)
    keep[rng.choice(len(s), d, replace=False)] = False
    return np.frombuffer(s, np.uint8)[keep].tobytes()


def insert_bytes(rng, s, d):
    out = bytearray(s)
    for _ in range(d):
        out.insert(int(rng.integers(0, len(out) + 1)), BASES[int(rng.integers(0, 4))])
    return bytes(out)


def border_positions(lengths, max_len, seed=20261501):
    """One position per template length (the reported maximum capped to it): 3 noisy reads, the template itself (d = 0), the
    template with d bytes deleted and with d bytes inserted (the lengths differ by exactly d either way: the walk runs along the
    band's edge), a read of one byte and a stranger that does not vote.  At the maximum the reads are cut to it."""
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        m = min(m, max_len)
        t = rand_seq(rng, m)
        d = min(max(1, m // 50), 40) if m > 1 else 0
        reads = [noisy(rng, t)[:max_len] for _ in range(1 if m >= max_len else 3)] + [t, delete_bytes(rng, t, d)]
        if m < max_len:
            reads += [insert_bytes(rng, t, max(d, 1)), t[:1], rand_seq(rng, m)]
        out.append((t, reads))
    return out


def many_reads_positions(counts, length=24, seed=20261502):
    rng = np.random.default_rng(seed)
    out = []
    for c in counts:
        t, reads, _ = position(rng, length, c, p_del=0.04, p_sub=0.04, p_ins=0.04)
        out.append((t, reads))
    return out


def many_positions(n, seed=20261503):
    """n positions of strings of at most 40 bytes; every seventh has no voting read, every eleventh no read at all."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(n):
        length = int(rng.integers(1, 36))
        t, reads, _ = position(rng, length, int(rng.integers(1, 5)), p_del=0.04, p_sub=0.04, p_ins=0.04)
        t = t[:40]
        reads = [r[:40] for r in reads]
        if p % 7 == 3:
            reads = [b"T" * 40 for _ in reads]
        if p % 11 == 5:
            reads = []
        out.append((t, reads))
    return out


def workload_position(seed, length=2055, n_reads=32):
    rng = np.random.default_rng(seed)
    return position(rng, length, n_reads)


# ---------------------------------------------------------------- device and restatement side by side
def pack(positions):
    t_off = np.zeros(len(positions) + 1, np.int64)
    np.cumsum([len(t) for t, _ in positions], out=t_off[1:])
    reads = [r for _, rs in positions for r in rs]
    r_off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=r_off[1:])
    pos_ptr = np.zeros(len(positions) + 1, np.int64)
    np.cumsum([len(rs) for _, rs in positions], out=pos_ptr[1:])
    return b"".join(t for t, _ in positions), t_off, b"".join(reads), r_off, pos_ptr


def device(engine, positions, n_iters=1, permille=300):
    """[[(output, voting, excluded) per position] per iteration] from one cf_consensus_run."""
    res = engine.consensus_run(*pack(positions), n_iters=n_iters, permille=permille)
    assert len(res) == n_iters
    out = []
    for b, off, nv, ne in res:
        assert off[0] == 0 and off[-1] == b.size and off.size == len(positions) + 1
        out.append([(b[off[p]:off[p + 1]].tobytes(), int(nv[p]), int(ne[p])) for p in range(len(positions))])
    return out


_expected = {}


def expected(positions, n_iters=1, permille=300):
    """The same from the restatement; computed once per input."""
    key = (tuple((bytes(t), tuple(bytes(r) for r in rs)) for t, rs in positions), n_iters, permille)
    if key not in _expected:
        per_pos = [consensus(t, rs, n_iters, permille) for t, rs in positions]
        _expected[key] = [[per_pos[p][i] for p in range(len(positions))] for i in range(n_iters)]
    return _expected[key]


def check(engine, positions, n_iters=2, permille=300):
    got, want = device(engine, positions, n_iters, permille), expected(positions, n_iters, permille)
    for i in range(n_iters):
        for p in range(len(positions)):
            assert got[i][p] == want[i][p], f"iteration {i + 1}, position index {p} (template of {len(positions[p][0])} bytes, {len(positions[p][1])} reads)"
    return got


def check_literals(engine):
    """Every literal case as a call of its own and all of one permille as one call."""
    for name, t, reads, permille, want in LITERALS:
        got = device(engine, [(t, reads)], len(want), permille)
        assert [g[0][0] for g in got] == list(want), name
        if name in LITERAL_COUNTS:
            assert got[0][0][1:] == LITERAL_COUNTS[name], name
    for permille in sorted({c[3] for c in LITERALS}):
        cases = [c for c in LITERALS if c[3] == permille]
        got = device(engine, [(c[1], c[2]) for c in cases], 1, permille)
        assert [g[0] for g in got[0]] == [c[4][0] for c in cases], permille


def check_refusals(engine, DeviceError):
    """-22 for each bad argument, the live device bytes as before, and a good call straight after."""
    import ctypes as C
    lib, ctx = engine._lib, engine._ctx
    good = [(b"ACGTACGTAC", [b"ACGTAGCGTAC", b"ACGTAGCGTAC", b"ACGTACGTAC"])]
    want = expected(good, 2, 300)
    assert device(engine, good, 2, 300) == want
    live = engine.stats()["hbm_bytes_live"]
    t, t_off, r, r_off, pos_ptr = pack(good)
    t, r = np.frombuffer(t, np.uint8), np.frombuffer(r, np.uint8)
    ms = C.c_float()

    def run(t_=t, t_off_=t_off, r_=r, r_off_=r_off, pos_ptr_=pos_ptr, n_iters=2, permille=300):
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.cf_consensus_run(ctx, p(t_), p(t_off_), p(r_), p(r_off_), p(pos_ptr_), 1, n_iters, permille, None, C.byref(ms))

    for kw, what in [(dict(t_off_=None), "null offsets"), (dict(r_off_=None), "null offsets"), (dict(pos_ptr_=None), "null offsets"),
                     (dict(t_=None), "null bytes"), (dict(r_=None), "null bytes"),
                     (dict(t_off_=np.array([10, 0], np.int64)), "decrease"), (dict(r_off_=np.array([0, 11, 5, 32], np.int64)), "decrease"),
                     (dict(pos_ptr_=np.array([0, -1], np.int64)), "decrease"), (dict(pos_ptr_=np.array([1, 3], np.int64)), "pos_ptr\\[0\\]"),
                     (dict(n_iters=0), "fewer than one iteration"), (dict(n_iters=-3), "fewer than one iteration"),
                     (dict(permille=-1), "negative divergence")]:
        import re
        assert run(**kw) == -22, kw
        assert re.search(what, lib.cf_last_error(ctx).decode()), (kw, lib.cf_last_error(ctx))
        assert engine.stats()["hbm_bytes_live"] == live, kw
        # the results of the call before are still there
        b = np.zeros(64, np.uint8)
        off = np.zeros(2, np.int64)
        assert lib.cf_consensus_get(ctx, 2, b.ctypes.data, off.ctypes.data, None, None) == 0
        assert b[:off[1]].tobytes() == want[1][0][0]
    assert lib.cf_consensus_get(ctx, 3, None, None, None, None) == -22 and lib.cf_consensus_get(ctx, 0, None, None, None, None) == -22
    assert device(engine, good, 2, 300) == want
    assert engine.stats()["hbm_bytes_live"] == live


def check_too_long(engine, DeviceError):
    """One byte above the reported maximum is refused, as a template and as a read, with a good call straight after."""
    import pytest
    max_len = engine.consensus_info()["max_len"]
    assert max_len >= 8192
    long = b"A" * (max_len + 1)
    live = engine.stats()["hbm_bytes_live"]
    with pytest.raises(DeviceError, match="template of position index 1 is longer") as ei:
        device(engine, [(b"ACGT", [b"ACGT"]), (long, [b"ACGT"])])
    assert "(-22)" in str(ei.value)
    with pytest.raises(DeviceError, match="read 2 is longer"):
        device(engine, [(b"ACGT", [b"ACGT", b"ACGT"]), (b"ACGT", [long])])
    assert engine.stats()["hbm_bytes_live"] == live
    check(engine, [(b"ACGT", [b"AGGT", b"AGGT", b"ACGT"])], 1, 1000)


def check_independence(engine):
    """The restatement's d is editcheck.nw and the device's own edit_distances on the same pairs: the three share no code."""
    import editcheck as ec
    rng = np.random.default_rng(20261504)
    pairs = [(t, r) for _, t, reads, _, _ in LITERALS for r in reads]
    for m in (1, 7, 33, 64, 130, 257):
        t = rand_seq(rng, m)
        pairs += [(t, noisy(rng, t, 0.05, 0.05, 0.05)), (t, rand_seq(rng, m + 3)), (t, t)]
    mine = [one_pass(t, [r], 10 ** 6)[3][0] for t, r in pairs]
    assert mine == [ec.nw(t, r) for t, r in pairs]
    aa, bb = b"".join(t for t, _ in pairs), b"".join(r for _, r in pairs)
    a_off = np.cumsum([0] + [len(t) for t, _ in pairs])
    b_off = np.cumsum([0] + [len(r) for _, r in pairs]) + len(aa)
    d, _ = engine.edit_distances(aa + bb, a_off, b_off)
    assert d.tolist() == mine and max(mine) > 100 and min(mine) == 0


def check_batches(engine):
    """cons_batch_bytes so small that the reads of one position span three batches and more, a position without a voting read in
    the middle of a batch; the bytes are those of the default batch."""
    rng = np.random.default_rng(20261505)
    t, reads, _ = position(rng, 60, 9, p_del=0.04, p_sub=0.04, p_ins=0.04)
    positions = [(t, reads), (rand_seq(rng, 50), [b"T" * 50, b"G" * 47]), many_reads_positions((4,), 60)[0]]
    want = check(engine, positions, 3)
    assert want[0][1][1:] == (0, 2)
    default = engine.consensus_info()
    for batch_bytes in (2048, 700, 1):
        with engine.knobs(cons_batch_bytes=batch_bytes):
            assert engine.consensus_info()["batch_bytes"] == batch_bytes
            assert check(engine, positions[:1], 3) == [w[:1] for w in want]
            assert engine.consensus_info()["n_batches"] >= 3 * 3
            assert check(engine, positions, 3) == want
            assert engine.consensus_info()["n_batches"] > default["n_batches"]
    assert engine.consensus_info()["batch_bytes"] == default["batch_bytes"]


def check_more_positions_than_the_launch_cap(engine):
    info = engine.consensus_info()
    positions = many_positions(info["launch_cap"] + 3)
    assert max(max([len(t)] + [len(r) for r in rs]) for t, rs in positions) <= 40
    got = check(engine, positions, 1)
    info = engine.consensus_info()
    assert info["n_reads"] > info["launch_cap"] and info["n_pos"] == len(positions)
    assert sum(1 for g, (t, rs) in zip(got[0], positions) if rs and g[1] == 0) >= 3      # positions whose reads all stay out


def check_hygiene(engine, DeviceError):
    """Two rounds of the same calls leave the same live device bytes (every scratch buffer goes back), two runs give the same bytes,
    nothing is added to cf_times or cf_stats."""
    positions = many_reads_positions((3, 5), 40)
    times, live = engine.times(), []
    res = []
    for _ in range(2):
        check_literals(engine)
        res.append(device(engine, positions, 3))
        try:
            device(engine, [(b"ACGT", [b"ACGT"])], 0)
        except DeviceError:
            pass
        live.append(engine.stats()["hbm_bytes_live"])
    assert live[0] == live[1] and res[0] == res[1] == expected(positions, 3)
    assert engine.times() == times


def check_tree(outdir, num_iters, permille=300):
    """What scripts/eltr_polisher.py --polisher consensus left in outdir against the restatement applied to the exported files."""
    import os
    import re
    import editcheck as ec
    from centroflye_amd import eltr_polisher as ep
    positions = sorted(int(d[4:]) for d in os.listdir(outdir) if d.startswith("pos_"))
    assert positions == list(range(positions[0], positions[-1] + 1))
    finals, rows = [""] * num_iters, []
    for pos in positions:
        d = os.path.join(outdir, f"pos_{pos}")
        t = ep.read_first_record(os.path.join(d, "median_read_unit.fasta")).encode()
        reads = [r.encode() for r in ep.read_records(os.path.join(d, "read_units.fasta"))]
        length = len(t)
        for i, per_pos in enumerate(expected([(t, reads)], num_iters, permille), 1):
            out, nv, ne = per_pos[0]
            with open(os.path.join(d, f"polished_{i}.fasta")) as f:
                assert f.read() == f">consensus_pos_{pos}_iter_{i}\n{out.decode()}\n", (pos, i)
            finals[i - 1] += out.decode()
            rows.append((i, pos, length, len(reads), nv, ne, len(out)))
            length = len(out)
        assert sorted(os.listdir(d)) == sorted(["median_read_unit.fasta", "read_units.fasta"] + [f"polished_{i}.fasta" for i in range(1, num_iters + 1)])
    for i in range(1, num_iters + 1):
        with open(os.path.join(outdir, f"final_sequence_{i}.fasta")) as f:
            assert f.read() == f">polished_repeat_{i}\n{finals[i - 1]}\n"
        with open(os.path.join(outdir, f"final_sequence_hpc_{i}.fasta")) as f:
            assert f.read() == f">polished_repeat_{i}\n{ec.hpc(finals[i - 1].encode()).decode()}\n"
    with open(os.path.join(outdir, "report.txt")) as f:
        dists = [int(x) for x in re.findall(r"'editDistance': (-?\d+)", f.read())]
    nw = lambda x, y: 0 if x == y else ec.nw(x, y)
    want = []
    for i in range(1, num_iters):
        x, y = finals[i - 1].encode(), finals[i].encode()
        want += [nw(x, y), nw(ec.hpc(x), ec.hpc(y))]
    assert dists == want
    with open(os.path.join(outdir, "consensus_report.tsv")) as f:
        lines = f.read().splitlines()
    assert lines[0].split("\t") == ["iteration", "position", "template_length", "reads", "voting", "excluded", "output_length"]
    assert [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:]] == sorted(rows)
    with open(os.path.join(outdir, "position_changes.csv")) as f:
        changes = [tuple(int(x) for x in ln.split(" ")) for ln in f.read().splitlines()]
    assert [c[:2] for c in changes] == [(i, pos) for i in range(1, num_iters) for pos in positions]
    return finals, rows

"""The device steps of the table exchange that only matter for more than one rank, on ONE engine, against a plain restatement.

Every -m gpu test of the sharded path opens a communicator of world 1, where cf_owner_of is always 0, every key reaches its owner
once and the reduced unique mask equals the local one.  Worlds 2, 3 and 8 run on the host emulator only, which takes ballots,
shuffles and atomics one lane after another.  Here the product's own kernels run for a VIRTUAL world, with no communicator:
  A  cf_xch_bucket_kernel (cf_selftest_owner_buckets): the table of cf_count_kmers, both layouts, bucketed for W = 1 .. 257 owners;
  B  cf_xch_merge_kernel (cf_selftest_merge_records): records whose keys arrive more than once, and the same records through the
     host-mediated twin cf_reset_table + cf_merge_table;
  C  one whole exchange: every virtual rank's shard counted and bucketed, every owner's buckets merged and selected, against
     shapecheck.naive_stage2 on the undivided reads;
  D  cf_merge_table's refusals and cf_or_unique_mask against numpy;
  E  (scratchcheck) the scratch balance of these calls.
The restatement is plain Python on ints, lists and dicts: mix64 from cf_common.h with 64-bit masks, owner(key, W) =
(mix64(key ^ 0x5bf03635) >> 33) % W from cf_exchange.hip, home(key, cap) = mix64(key) & (cap - 1).  (Where a table has half a
million keys the per-owner grouping of the restated owners is done by numpy sorts; the hash itself never is.)  `wrong=` makes the
restatement subtly wrong (WRONG below): test_emu_exchange.py asserts that the comparison then FAILS.  Every case carries a regime
check evaluated on the restatement alone, BEFORE the device is asked.  All comparisons are integer-exact.
Used by test_emu_exchange.py (host emulator) and test_gpu_exchange.py (MI355X)."""
import functools
from collections import Counter

import numpy as np

import shapecheck
from centroflye_amd.engine import DeviceError

M64 = (1 << 64) - 1
OWNER_SALT = 0x5bf03635
XCH_THREADS = 256             # threads of a workgroup of cf_xch_bucket_kernel, and the slots it takes per step
WORLDS = (1, 2, 3, 8, 64, 65, 257)
WRONG = ("shift32", "overwrite", "multi_low", "run_start")
MAX_KEY = (1 << 62) - 1       # poly-T at k = 31


def mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x


def owner(key, W, wrong=None):
    return (mix64(key ^ OWNER_SALT) >> (32 if wrong == "shift32" else 33)) % W


def home(key, cap):
    return mix64(key) & (cap - 1)


def pow2_ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


# ------------------------------------------------------------------ A: the table bucketed by owner
def naive_table(reads, k):
    """{code: [pres, multi]} of A1 (distance_based_kmer_recruitment.py:39-63) on plain reads."""
    table = {}
    for r in reads:
        for w, f in Counter(r[i:i + k] for i in range(len(r) - k + 1)).items():
            assert shapecheck.plain(w)
            e = table.setdefault(shapecheck.code_of(w), [0, 0])
            e[0] += 1
            e[1] += f > 1
    return table


def expected_buckets(table, W, wrong=None, cache=None):
    """table {key: [pres, multi]} -> (start[W + 1], keys, vals, owners): the records in owner-major order, by key inside an
    owner.  wrong="run_start": the first run that does not begin the buffer starts one record late.  cache: a dict that keeps
    the hashes of the table's keys from one W to the next."""
    cache = {} if cache is None else cache
    if wrong not in cache:
        keys = sorted(table)
        shift = 32 if wrong == "shift32" else 33
        cache[wrong] = (np.array(keys, np.uint64), np.array([table[key][0] | table[key][1] << 32 for key in keys], np.uint64),
                        [mix64(key ^ OWNER_SALT) >> shift for key in keys])
    ka, va, hashes = cache[wrong]
    assert not hashes or [hashes[0] % W, hashes[-1] % W] == [owner(int(ka[0]), W, wrong), owner(int(ka[-1]), W, wrong)]
    oa = np.array([h % W for h in hashes], np.int64)
    start = [0]
    for c in np.bincount(oa, minlength=W).tolist():
        start.append(start[-1] + c)
    if wrong == "run_start":
        o = next(o for o in range(1, W) if 0 < start[o] < start[o + 1])
        start[o] += 1
    order = np.lexsort((ka, oa))
    return np.array(start, np.int64), ka[order], va[order], oa[order]


def check_buckets(engine, table, W, what, regime=None, wrong=None, cache=None):
    """The table the engine holds (restated: `table`) bucketed for W owners: start, and every owner's run as a multiset."""
    start, keys, vals, own = expected_buckets(table, W, wrong, cache)
    if regime:
        regime(W, np.diff(start))
    g_start, g_keys, g_vals = engine.selftest_owner_buckets(W)
    n = len(table)
    assert g_start.size == W + 1 and g_start[0] == 0 and g_start[W] == n and (np.diff(g_start) >= 0).all(), f"{what}, W={W}: start {g_start}"
    assert g_keys.size == n and g_vals.size == n, f"{what}, W={W}: {g_keys.size} records for {n} keys"
    assert np.array_equal(g_start, start), f"{what}, W={W}: start"
    seg = np.repeat(np.arange(W, dtype=np.int64), np.diff(g_start))          # the run each record lies in
    order = np.lexsort((g_keys, seg))
    assert np.array_equal(seg[order], own), f"{what}, W={W}: a record lies in another owner's run"
    assert np.array_equal(g_keys[order], keys), f"{what}, W={W}: keys of the runs"
    assert np.array_equal(g_vals[order], vals), f"{what}, W={W}: pres | multi << 32 of the runs"
    return g_start, g_keys, g_vals


@functools.lru_cache(maxsize=None)
def de_bruijn(k):
    """A de Bruijn sequence B(4, k) as ACGT bytes, its first k - 1 bases once more behind it: 4^k windows, all different (the
    concatenation of the Lyndon words whose length divides k, in order).  It starts with poly-A."""
    seq, w = [], [-1]
    while w:
        w[-1] += 1
        m = len(w)
        if k % m == 0:
            seq.extend(w)
        while len(w) < k:
            w.append(w[-m])
        while w and w[-1] == 3:
            w.pop()
    s = bytes(seq).translate(bytes.maketrans(bytes(range(4)), b"ACGT"))
    return s + s[:k - 1]


def dense_case(n):
    """Reads with exactly n distinct k-mers: a prefix of a de Bruijn sequence cut into two reads that share no window, and (from
    n = 63) a third read that holds three of its windows twice (pres 2, multi 1) and k - 1 windows of its own at the joint."""
    k = 6
    while 4 ** k < n + n // 4:
        k += 1
    s = de_bruijn(k)
    if n < 63:
        reads = [s[:n + k - 1]]
    else:
        extra = s[:k + 2] * 2
        at = [s.find(extra[i:i + k]) for i in range(len(extra) - k + 1)]          # (a window of s stands at one place)
        m = next(m for m in range(max(n - len(at), 8), n + 1) if m + len({extra[i:i + k] for i, p in enumerate(at) if p < 0 or p >= m}) == n)
        reads = [s[:m // 2 + k - 1], s[m // 2:m + k - 1], extra]

    def regime(table):
        assert len(table) == n, (len(table), n)
        if n >= 63:
            assert max(e[0] for e in table.values()) == 2 and sum(e[1] for e in table.values()) >= 3
        else:
            assert 0 in table           # poly-A: code 0
    return dict(name=f"dense table of {n} keys, k={k}", reads=reads, k=k, count_mode=1, regime=regime, all_owners_to=8 if n >= 63 else 0,
                empty_at_257=n <= 257)


def dense_sizes(g):
    """g: workgroups of the launch (8 per CU).  A last wave partly past the table's end, one workgroup with a single slot (the
    chunk of 256 g + 1 slots over g workgroups is 512: workgroup g / 2 gets one), workgroups whose chunk starts past the end."""
    return (1, 63, 64, 65, 255, 256, 257, XCH_THREADS * g + 1)


def hash_case(n_windows, k, seed):
    """The probed table of cf_count.hip (count_mode 0): pow2_ceil(max(windows, 1024)) slots."""
    read = shapecheck.rand_seq(np.random.default_rng(seed), n_windows + k - 1)

    def regime(table):
        assert len(table) == n_windows and pow2_ceil(max(n_windows, 1024)) == (1024 if n_windows <= 1024 else 4096)
    return dict(name=f"hash table of {n_windows} keys", reads=[read], k=k, count_mode=0, regime=regime, all_owners_to=8 if n_windows > 100 else 0,
                empty_at_257=n_windows <= 257)


def extremes_case():
    """poly-A (code 0: only CF_OCC tells the slot from an empty one) and poly-T (2^62 - 1) at k = 31, among other k-mers."""
    reads = [b"A" * 40, b"T" * 35, shapecheck.rand_seq(np.random.default_rng(31), 60)]

    def regime(table):
        assert table[0] == [1, 1] and table[MAX_KEY] == [1, 1] and len(table) == 32
    return dict(name="poly-A and poly-T at k=31", reads=reads, k=31, count_mode=1, regime=regime, all_owners_to=3, empty_at_257=True)


def check_table_case(engine, case, worlds=WORLDS, wrong=None):
    """Part A on one table: load, count, and the buckets of every W.  The regime per W: every owner holds a key up to
    W = case["all_owners_to"] (8 for the tables of 63 keys or more; a table of 1, 5 or 32 keys cannot fill 8 owners), and W = 257 has
    empty owners beside full ones where case["empty_at_257"] (tables of up to 257 keys)."""
    what = case["name"]
    table = case.get("table") or naive_table(case["reads"], case["k"])
    case["table"] = table
    case["regime"](table)                                 # from the reads alone, before the device is asked

    def regime(W, sizes):
        if W <= case["all_owners_to"]:
            assert (sizes > 0).all(), f"{what}: an owner of {W} has no key"
        if W == 257 and case["empty_at_257"]:
            assert (sizes == 0).any() and (sizes > 0).any()
    with engine.knobs(count_mode=case["count_mode"]):
        engine.load_arrays(*shapecheck.to_arrays(case["reads"], [[] for _ in case["reads"]]))
        engine.count_kmers(case["k"])
    keys, pres, multi = engine.table()
    want = sorted(table)
    assert np.array_equal(keys, np.array(want, np.uint64)), f"{what}: A1 keys"
    assert pres.tolist() == [table[x][0] for x in want] and multi.tolist() == [table[x][1] for x in want], f"{what}: A1 counts"
    for W in worlds:
        start, gk, _ = check_buckets(engine, table, W, what, regime, wrong, case.setdefault("hashes", {}))
        for x in (0, MAX_KEY):                            # the extreme keys, each in the run of its restated owner
            if x in table:
                o = owner(x, W)
                assert (gk[start[o]:start[o + 1]] == np.uint64(x)).any(), f"{what}, W={W}: key {x} is not with owner {o}"


# ------------------------------------------------------------------ B: records merged into the owner's table
def expected_merge(recs, wrong=None):
    """recs: (key, pres, multi) -> {key: val}, val = sum of pres | sum of multi << 32."""
    out = {}
    for key, pres, multi in recs:
        p, m = out.get(key, (0, 0))
        if wrong == "overwrite":
            p, m = 0, 0
        if wrong == "multi_low":
            p, multi = p + multi, 0
        out[key] = (p + pres, m + multi)
    return out


def _read_table(engine):
    keys, pres, multi = engine.table()
    return {int(x): (int(p), int(m)) for x, p, m in zip(keys.tolist(), pres.tolist(), multi.tolist())}, keys.size


def check_merge(engine, case, wrong=None, parts=None):
    """parts None: cf_selftest_merge_records (cf_xch_merge_kernel); parts p: cf_reset_table + p calls of cf_merge_table."""
    recs, what = case["recs"], case["name"]
    want = expected_merge(recs, wrong)
    case["regime"](want)
    assert all(p < 1 << 32 and m < 1 << 32 for p, m in want.values()), f"{what}: a sum leaves its half of the value"
    keys = np.array([r[0] for r in recs], np.uint64)
    pres = np.array([r[1] for r in recs], np.uint64)
    multi = np.array([r[2] for r in recs], np.uint64)
    if parts is None:
        engine.selftest_merge_records(keys, pres | multi << np.uint64(32))
    else:
        engine.reset_table(31, len(recs))
        cuts = [len(recs) * i // parts for i in range(parts + 1)]
        for a, b in zip(cuts, cuts[1:]):
            engine.merge_table(keys[a:b], pres[a:b].astype(np.uint32), multi[a:b].astype(np.uint32))
    got, n = _read_table(engine)
    assert n == len(got) == len(want), f"{what}: {n} slots for {len(want)} keys"
    assert got == want, f"{what}: {sum(got.get(x) != v for x, v in want.items())} of {len(want)} keys differ"


def _some_keys(n, seed):
    keys = sorted({int(x) for x in np.random.default_rng(seed).integers(1, MAX_KEY, n + 8)})[:n]
    assert len(keys) == n
    return keys


def copies_case(V, order):
    """V copies of each of 300 keys; order: "adjacent" (all copies of a key next to each other: one wave), "blocks" (copy v of every
    key in block v: far apart), "shuffle"."""
    keys = _some_keys(300, 300 + V)
    recs = [(x, 1 + (7 * i + v) % 50, (i + v) % 3) for i, x in enumerate(keys) for v in range(V)]
    if order == "blocks":
        recs = [recs[i * V + v] for v in range(V) for i in range(len(keys))]
    elif order == "shuffle":
        recs = [recs[i] for i in np.random.default_rng(V).permutation(len(recs))]

    def regime(want):
        assert len(want) == 300 and len(recs) == 300 * V
        if order == "adjacent":
            assert all(recs[i][0] == recs[i - i % V][0] for i in range(len(recs)))
        if order == "blocks":
            assert [r[0] for r in recs[:300]] == keys and [r[0] for r in recs[300:600]] == keys
    return dict(name=f"{V} copies of 300 keys, {order}", recs=recs, regime=regime)


def carry_case():
    """Sums of pres of 2^31 .. 2^32 - 1 with multi not 0: nothing may carry into the high half."""
    keys = _some_keys(48, 48)
    recs = []
    for i, x in enumerate(keys):
        top = (1 << 32) - 1 - (i % 3) * ((1 << 31) - 1) // 2         # 2^32 - 1 for every third key, down to 2^31
        parts = [top // 2, top // 3, top - top // 2 - top // 3]
        recs += [(x, p, 1 + (i + v) % 4) for v, p in enumerate(parts)]
    recs = [recs[i] for i in np.random.default_rng(2).permutation(len(recs))]

    def regime(want):
        sums = [p for p, _ in want.values()]
        assert min(sums) >= 1 << 31 and max(sums) == (1 << 32) - 1 and all(m >= 3 for _, m in want.values())
    return dict(name="low-half sums up to 2^32 - 1", recs=recs, regime=regime)


def wrap_case():
    """9 keys whose home in a table of 1024 slots is 1021, 1022 or 1023, each twice: the probe chain goes on at slot 0."""
    keys, x = [], 0
    while len(keys) < 9:
        x += 1
        if home(x, 1024) >= 1021:
            keys.append(x)
    recs = [(x, 3 + i, i % 2) for i, x in enumerate(keys)] + [(x, 100 + i, 1) for i, x in enumerate(reversed(keys))]

    def regime(want):
        assert len(want) >= 8 and len(recs) <= 512 and pow2_ceil(max(2 * len(recs), 1024)) == 1024
        assert all(home(x, 1024) in (1021, 1022, 1023) for x in want) and len(want) > 3
    return dict(name="probe chains that wrap to slot 0", recs=recs, regime=regime)


def empty_case():
    def regime(want):
        assert want == {}
    return dict(name="no records", recs=[], regime=regime)


def extreme_records_case():
    recs = [(0, 5, 1), (MAX_KEY, 7, 0), (MAX_KEY, 1, 2), (0, 2, 0)]

    def regime(want):
        assert want == {0: (7, 1), MAX_KEY: (8, 2)}
    return dict(name="codes 0 and 2^62 - 1, each twice", recs=recs, regime=regime)


def merge_cases():
    return ([copies_case(V, order) for V in (2, 8) for order in ("adjacent", "blocks", "shuffle")]
            + [carry_case(), wrap_case(), empty_case(), extreme_records_case()])


# ------------------------------------------------------------------ C: a whole exchange with virtual ranks
SHARDS = {2: (20, 20), 3: (5, 25, 10), 8: (7, 0, 9, 3, 0, 12, 8, 1)}
EXCHANGE = dict(k=11, max_nonuniq=3, lo=3, hi=12)


@functools.lru_cache(maxsize=None)
def exchange_reads():
    """40 reads of 6 units of 50 bases: copies of one array in which unit 4 begins like unit 1 (k-mers twice in a read), with 14
    variant sites that 3 .. 10 reads share (k-mers of a middling presence, spread over the shards) and a few private substitutions."""
    rng = np.random.default_rng(40)
    base = bytearray(shapecheck.rand_seq(rng, 300))
    base[200:230] = base[50:80]
    sites = [(int(rng.integers(0, 300)), rng.choice(40, int(rng.integers(3, 11)), replace=False).tolist()) for _ in range(14)]
    reads = []
    for r in range(40):
        b = bytearray(base)
        for pos, who in sites:
            if r in who:
                b[pos] = b"ACGT"[(b"ACGT".index(base[pos]) + 1) % 4]
        for pos in rng.integers(0, 300, 2).tolist():
            b[pos] = b"ACGT"[(b"ACGT".index(b[pos]) + 2) % 4]
        reads.append(bytes(b))
    units = [[(50 * u, 50 * u + 50) for u in range(6)] for _ in reads]
    p = EXCHANGE
    nv = shapecheck.naive_stage2(reads, units, p["k"], p["max_nonuniq"], p["lo"], p["hi"], max_pairs=0)
    return reads, units, nv


def check_exchange(engine, W, wrong=None):
    reads, units, nv = exchange_reads()
    p = EXCHANGE
    k = p["k"]
    sizes = SHARDS[W]
    cuts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert cuts[-1] == len(reads) and len(sizes) == W
    shard = [naive_table(reads[a:b], k) for a, b in zip(cuts, cuts[1:])]
    glob = {int(x): [int(pr), int(mu)] for x, pr, mu in zip(nv["keys"].tolist(), nv["pres"].tolist(), nv["multi"].tolist())}
    rare = set(nv["set_codes"].tolist())
    # the regime, from the restatement alone
    assert sum(1 for x in glob if sum(x in t for t in shard) >= 2) > 100, "no key has contributions of two ranks"
    hidden = [x for x in rare if all(not (x in t and t[x][1] <= p["max_nonuniq"] and p["lo"] <= t[x][0] <= p["hi"]) for t in shard)]
    assert hidden, "every globally rare key is rare within some shard"
    assert len(rare) > 20 and (W != 8 or 0 in sizes) and (W != 3 or len(set(sizes)) == 3)
    assert any(e[1] > p["max_nonuniq"] for e in glob.values()), "no key is cut by its multi-occurrence count"
    # every rank: count its shard, bucket the table; the buckets stay on the host
    sent = []
    for r, (a, b) in enumerate(zip(cuts, cuts[1:])):
        engine.load_arrays(*shapecheck.to_arrays(reads[a:b], units[a:b]))
        engine.count_kmers(k)
        sent.append(check_buckets(engine, shard[r], W, f"exchange, rank {r} of {W}"))
    # every owner: the buckets of all ranks in rank order, merged; the global counts of its keys; its rare k-mers
    found = []
    for o in range(W):
        gk = np.concatenate([kk[st[o]:st[o + 1]] for st, kk, _ in sent])
        gv = np.concatenate([vv[st[o]:st[o + 1]] for st, _, vv in sent])
        engine.selftest_merge_records(gk, gv)
        got, n = _read_table(engine)
        want = {x: tuple(e) for x, e in glob.items() if owner(x, W, wrong) == o}
        assert n == len(got) and got == want, f"exchange, owner {o} of {W}: the merged table is not the global count of its keys"
        n_sel = engine.select_rare(p["max_nonuniq"], p["lo"], p["hi"])
        mine = engine.kmers()
        assert n_sel == mine.size == sum(1 for x in rare if owner(x, W, wrong) == o), f"exchange, owner {o} of {W}: rare k-mers"
        found.append(mine)
    assert np.array_equal(np.sort(np.concatenate(found)), nv["set_codes"]), f"exchange, W={W}: the union of the owners' rare lists"


# ------------------------------------------------------------------ D: the host-mediated twins
def check_merge_table_refusals(engine, fresh):
    """fresh: an engine that has no table yet."""
    def refused(e, code, word, call):
        try:
            call()
        except DeviceError as err:
            assert f"({code})" in str(err) and word in str(err), str(err)
        else:
            raise AssertionError(f"cf_merge_table was not refused ({word})")
    one = (np.array([5], np.uint64), np.array([1], np.uint32), np.array([0], np.uint32))
    refused(fresh, -22, "no table", lambda: fresh.merge_table(*one))
    case = dense_case(63)
    engine.load_arrays(*shapecheck.to_arrays(case["reads"], [[] for _ in case["reads"]]))
    engine.count_kmers(case["k"])
    refused(engine, -22, "cf_reset_table", lambda: engine.merge_table(*one))
    engine.reset_table(31, 0)
    keys = np.arange(1, 1026, dtype=np.uint64) * np.uint64(1000003)
    assert np.unique(keys).size == 1025 and int(keys.max()) <= MAX_KEY
    refused(engine, -34, "table full", lambda: engine.merge_table(keys, np.ones(1025, np.uint32), np.zeros(1025, np.uint32)))
    first = merge_cases()[0]
    check_merge(engine, first)
    check_merge(engine, first, parts=2)


MASK_SIZES = (31, 32, 33, 64, 2049)


def check_or_unique_mask(engine, n):
    """cf_or_unique_mask on a set of n k-mers against numpy's OR, with stats()["n_unique"]."""
    engine.set_kmers(np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1), 11)
    rng = np.random.default_rng(n)
    cur = np.zeros(n, bool)

    def step(mask, what, changes):
        nonlocal cur
        mask = np.asarray(mask, bool)
        assert bool((mask & ~cur).any()) == changes, f"{n} k-mers, {what}: the mask lost its purpose"
        cur = cur | mask
        engine.or_unique_mask(mask)
        assert np.array_equal(engine.unique_mask(), cur), f"{n} k-mers: unique mask after {what}"
        assert engine.stats()["n_unique"] == int(cur.sum()), f"{n} k-mers: n_unique after {what}"
    assert engine.stats()["n_unique"] == 0 and not engine.unique_mask().any()
    step(np.zeros(n, bool), "an empty mask", False)
    step(rng.random(n) < 0.3, "a random mask", True)
    step(cur & (rng.random(n) < 0.5), "bits that are set already", False)
    step(np.zeros(n, bool), "an empty mask on set bits", False)
    engine.reset_unique()
    cur = np.zeros(n, bool)
    assert engine.stats()["n_unique"] == 0 and not engine.unique_mask().any()
    edge = np.zeros(n, bool)
    edge[[i for i in (31, 32, n - 1) if i < n]] = True      # the last bit of a word, the first of the next, the last k-mer
    step(edge, "bits on both sides of a word border", True)
    half = np.arange(n) % 2 == 0
    step(half, "every other bit", True)
    step(np.ones(n, bool), "all ones", True)
    step(np.ones(n, bool), "all ones again", False)
    engine.reset_unique()
    cur = np.zeros(n, bool)
    step(edge, "the border bits after a reset", True)

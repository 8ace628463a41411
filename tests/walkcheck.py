"""cf_group_walk_kernel with the open group's union in an LDS table unit -> bit (knob dist_walk), on hand-built reads at the
shapes where the table can go wrong, and the kernel it replaced (dist_walk 0) on the same reads: every case of tests/setupcheck.py and
the cases below, against the plain restatement (setupcheck.run: edges, n_edges, n_emissions, unique mask against
shapecheck.naive_stage2, n_dist_passes against groupcheck.expected_passes).

The table, restated: DIST_WALK_TAB = 64 slots, home slot (unit * 0x9E3779B1 mod 2^32) >> 26, linear probing that wraps; a cut empties it.
Every case proves its shape FROM NUMPY ALONE before the device runs.
Used by test_emu_dist_walk.py (host emulator) and test_gpu_dist_walk.py (MI355X)."""
import groupcheck as gc
import setupcheck as sc
import shapecheck  # noqa: F401  (the restatement every case is checked against, through setupcheck.run)

TAB = 64
KNOB = (1, 0)


def _home(unit):
    """The home slot of a unit in the walk's table (cf_walk_home of cf_dist.hip), restated."""
    return ((unit * 0x9E3779B1) & 0xFFFFFFFF) >> 26


def slots_of(union):
    """Where the postings of a union, in their order of joining, come to stand: {unit: (home, slot)}."""
    used, out = {}, {}
    for u in union:
        s = _home(u)
        while s in used:
            s = (s + 1) % TAB
        used[s] = u
        out[u] = (_home(u), s)
    return out


def collision_case():
    """One group whose union holds three postings with home slot 63 — their chain wraps the table's end — and one with home 0 that
    does not stand there (the head unit or the chain took the slot).  M0 brings the three, M1 finds the chain's last and brings the displaced one, M2 finds the middle one and the
    displaced one, M3 only the head unit and the first of the chain."""
    pool = 400
    unit = lambda q: 2 + 2 * q      # noqa: E731  (before = 0: the head read has the units 0 and 1, pool read q the units 2 + 2 q and 3 + 2 q)
    at63 = [q for q in range(1, pool) if _home(unit(q)) == 63][:3]
    at0 = [q for q in range(1, pool) if _home(unit(q)) == 0][:1]
    assert len(at63) == 3 and len(at0) == 1, "the pool holds the colliding units"
    a, b, c_ = at63
    (d,) = at0
    lists = {(0, 0): [0, a, b, c_], (0, 1): [0, c_, d], (0, 2): [0, b, d], (0, 3): [0, a]}      # (pool read 0 in every list: the second posting, so the members stand in the order of their numbers)
    c = sc.runs_case((4,), before=0, pool=pool, lists=lists, name="postings that collide in the walk's table, a chain that wraps")
    assert [c["unit_of"](1 + q, 0) for q in (a, d)] == [unit(a), unit(d)], "pool read q stands where the homes were computed"
    (g,) = [g for g in gc.groups_of(c["naive"]) if set(g[0]) & set(c["planted"][0])]
    assert g[0] == tuple(c["planted"][0]), "one group, the members in the order of their numbers"
    where = slots_of(g[1])
    chain = [where[unit(q)] for q in (a, b, c_)]
    slots = sorted(s for _, s in chain)
    assert [h for h, _ in chain] == [63, 63, 63] and slots[2] == 63 and slots[1] < 8, ("three postings of one home: two of them stand beyond the table's end, at its beginning", chain)
    assert where[unit(d)][0] == 0 and where[unit(d)][1] != 0, ("a posting that does not stand at its home", where[unit(d)])
    return c


def window_cuts_case():
    """A run of 130 from position 0 that the union cuts exactly in front of the members 64 and 128: a window of the walk ends and a group
    with it.  Members 0 .. 63 have two postings beyond the head unit out of nine; member 64 brings 31 others (with the head unit: a union
    of 32 by itself), 65 .. 127 are subsets of it; member 128 the same once more."""
    lists = {}
    for m in range(130):
        base = 40 * (m // 64)
        lists[(0, m)] = list(range(base, base + 31)) if m in (64, 128) else [base, base + 1 + m % 8]
    c = sc.runs_case((130,), before=0, pool=120, lists=lists, name="cuts by the union at the borders of the walk's windows")
    order = sc.order_of(c)
    assert order[:130] == c["planted"][0], "the members stand in the order of their numbers, from position 0"
    starts = [order.index(g[0][0]) for g in gc.groups_of(c["naive"]) if set(g[0]) & set(c["planted"][0])]
    assert starts == [0, 64, 128], starts
    return c


NEW = {
    "table_collisions_and_wrap": lambda e: sc.run(e, collision_case()),
    "cuts_at_window_borders": lambda e: sc.run(e, window_cuts_case()),
    "cuts_at_window_borders_cap_5": lambda e: sc.run(e, window_cuts_case(), cap=5),
}
NEW.update({f"caps_group_cap_{k}": (lambda k: lambda e: sc.run(e, sc.caps_case(), cap=k))(k) for k in (1, 2, 5, 32)})
NEW.update({f"table_collisions_group_cap_{k}": (lambda k: lambda e: sc.run(e, collision_case(), cap=k))(k) for k in (2, 5)})


def run_new(engine, name, knob):
    with engine.knobs(dist_walk=knob):
        NEW[name](engine)


def run_setup_knob_0(engine, name):
    """A case of tests/setupcheck.py on the kernel that keeps the union in the lanes (the knob at 1 is what test_*_dist_setup.py runs)."""
    with engine.knobs(dist_walk=0):
        sc.CASES[name](engine)


def run_not_sets(engine, knob):
    with engine.knobs(dist_walk=knob):
        gc.run_repeated_rank(engine)

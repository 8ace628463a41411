"""What follows the graph in centroflye_amd/debruijn_graph.py — map_reads (cf_monomap.hip on the host emulator), index_edges,
scaffolding, read2scaffolds, cover_scaffolds_w_reads, partition_pseudounits, extract_read_pseudounits — and the driver's files
against what the reference's modules made of the same inputs (tests/golden/mono_scaffold_cases.json, captured by
tools/capture_mono_scaffold_cases.py; the inputs and the record format are in tests/monoscaffoldcheck.py)."""
import json
import os
import random
import types

import pytest

import monoscaffoldcheck as sc
from centroflye_amd import debruijn_graph, mono_error_correction, sd_parser, session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "mono_scaffold_cases.json")) as f:
    GOLDEN = json.load(f)
MODS = types.SimpleNamespace(MonoString=sd_parser.MonoString, split=mono_error_correction.split_monostring, ec=mono_error_correction, graph=debruijn_graph)


@pytest.fixture(scope="module")
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


def strip(case):
    return {k: v for k, v in case.items() if k != "want"}


def ident(case):
    return case["name"][:40].replace(" ", "_")


def test_the_fixture_holds_the_cases_the_tool_would_write_today():
    rng = random.Random(33)
    assert [strip(c) for c in GOLDEN["pipeline"]] == json.loads(json.dumps(sc.pipeline_cases(rng)))
    assert [strip(c) for c in GOLDEN["scaffolding"]] == json.loads(json.dumps(sc.scaffolding_cases()))
    assert [s for s, _ in GOLDEN["partition"]] == sc.PARTITION_STRINGS
    assert GOLDEN["e2e"]["spec"] == json.loads(json.dumps(sc.E2E)) and set(GOLDEN["e2e"]["files"]) == set(sc.FILES)


def test_the_cases_cover_the_issues_list():
    names = " | ".join(c["name"] for c in GOLDEN["scaffolding"])
    for what in ("ties in the longest path", "cyclic component", "exactly two reads", "min_connections 1", "min_connections 3", "additional_edges", "equal support",
                 "left and right extensions", "smaller than half"):
        assert what in names, what
    by = {c["name"]: c["want"] for c in GOLDEN["scaffolding"]}
    chain = by["a chain of three long edges; left and right extensions, the longest wins, the first of equal ones stays"]
    # the longer left extension (two edges) wins; of the two right extensions of one edge each the first one found stays
    assert chain["edge_scaffolds"] == [[8, 7, 0, 1, 2, 3, 4, 5]] and chain["scaffolds"] == ["JllGlAaaBCbbDcEddFrH"]
    # no link: every long edge is a scaffold of its own, extended by the reads that pass it
    assert by["min_connections 3 is missed by two reads"]["edge_scaffolds"] == [[0, 1, 2], [0, 1, 2, 3, 4], [2, 3, 4]]
    assert by["min_connections met by exactly two reads"]["edge_scaffolds"] == [[0, 1, 2, 3, 4], [2, 3, 4]]
    assert by["min_connections 1 links what one read supports"]["edge_scaffolds"] == [[0, 1, 2, 3, 4]]
    assert by["a cyclic component is skipped, its neighbours are not"]["edge_scaffolds"] == [[2, 3], [4]]
    assert by["two connections with equal support: the first one found fills the link"]["edge_scaffolds"] == [[0, 2, 3]]
    assert by["the better supported connection fills the link"]["edge_scaffolds"] == [[0, 2, 3]]
    fig = GOLDEN["e2e"]["figures"]
    assert fig["scaffolds"] >= 1 and fig["covered_pseudounits"] >= 1 and fig["long_edges"] >= 1 and max(fig["long_edges_per_scaffold"]) >= 2


@pytest.mark.parametrize("case", GOLDEN["scaffolding"], ids=ident)
def test_scaffolding_equals_the_reference(case):
    assert sc.run_scaffolding(MODS, case) == case["want"]


def test_partition_pseudounits_equals_the_reference():
    assert sc.run_partition(MODS) == GOLDEN["partition"]


@pytest.mark.parametrize("case", GOLDEN["pipeline"], ids=ident)
def test_the_pipeline_behind_the_graph_equals_the_reference(emu_session, case, tmp_path):
    got = sc.run_pipeline(MODS, case, str(tmp_path))
    for key in case["want"]:
        assert got[key] == case["want"][key], key
    assert set(got) == set(case["want"])


def test_the_first_pipeline_case_holds_what_it_is_there_for(emu_session, tmp_path):
    """the long values of the fixture are SHA-1s: the unshrunk record, pinned to the fixture first, is looked at here"""
    import monographcheck as gc
    case = GOLDEN["pipeline"][0]
    raw = sc.run_pipeline(MODS, case, str(tmp_path), raw=True)
    assert gc.shrink_all(raw) == case["want"]
    maps, placed, cover = raw["map_reads"], raw["read2scaffolds"], raw["cover_scaffolds_w_reads"]
    assert maps['"alien"'] is None and maps['"short"'] is None and maps['"empty"'] is None      # no hit
    assert maps['"jump"'][2] is False and len(maps['"jump"'][3]) == 2                           # an invalid path
    assert maps['"gap"'][2] is True and maps['"gap"'][0][2] == 0 and maps['"gap"'][1][2] > 5    # positions count the gap
    assert len(raw["scaffolding"]["edge_scaffolds"]) == 1 and len(raw["scaffolding"]["edge_scaffolds"][0]) == 5
    assert len(maps['"inrep"'][3]) == 1 and '"inrep"' not in placed                             # the repeat fits two places: dropped
    assert '"del"' in placed and not any('"del"' in at for s in cover for at in s)              # the spans differ: skipped
    # a cut read: the first part has its whole map, the second part what the truncated map still holds, the third nothing
    on = lambda key: sum(key in at for s in cover for at in s)      # noqa: E731
    assert all(key in placed for key in ('["cut", 0]', '["cut", 1]', '["cut", 2]')) and (on('["cut", 0]'), on('["cut", 1]'), on('["cut", 2]')) == (9, 2, 0)
    assert any(len(unit) >= 2 for s in raw["extract_read_pseudounits_2"]["read_pseudounits"] for unit in s)


def test_map_reads_leaves_a_stale_index_alone(emu_session):
    """on purpose: map_reads neither builds nor reads db_index"""
    case = GOLDEN["pipeline"][0]
    reads = sc.make_reads(MODS, case)
    db = sc.build_db(MODS, case, reads, None)
    mapping = db.map_reads(reads, verbose=False)
    assert not hasattr(db, "db_index")
    db.db_index = {"stale": True}
    assert db.map_reads(reads, verbose=False) == mapping and db.index_edges() == {"stale": True}


def test_the_driver_writes_the_reference_s_results(emu_session, tmp_path):
    sc.check_end_to_end(tmp_path, GOLDEN["e2e"])

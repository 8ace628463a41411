"""mono_error_correction.split_monostring (the reference's MonoString.split), centroflye_amd/mono_error_correction.py and centroflye_amd/debruijn_graph.py against what the reference's modules
made of the same inputs (tests/golden/mono_graph_cases.json, captured by tools/capture_mono_graph_cases.py; the inputs and the
record format are in tests/monographcheck.py), with the k-mer counts coming from cf_monokmers.hip on the host emulator."""
import json
import os
import types

import pytest

import monographcheck as gc
from centroflye_amd import debruijn_graph, mono_error_correction, sd_parser, session
from centroflye_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "mono_graph_cases.json")) as f:
    GOLDEN = json.load(f)
# the cases on the large read set take minutes on the emulator: they run on the GPU (tests/test_gpu_mono_graph.py)
SMALL = {sec: [c for c in GOLDEN[sec] if "strings_seed" not in c] for sec in ("graph", "iterative")}
MODS = types.SimpleNamespace(MonoString=sd_parser.MonoString, split=mono_error_correction.split_monostring, ec=mono_error_correction, graph=debruijn_graph)


@pytest.fixture(scope="module")
def emu_session(emu_lib):
    session.reset()
    session._engine = Engine(0, emu_lib)
    yield session
    session.reset()


def strip(case):
    return {k: v for k, v in case.items() if k != "want"}


def test_the_fixture_holds_the_cases_the_tool_would_write_today():
    import random
    rng = random.Random(29)
    assert [strip(c) for c in GOLDEN["split"]] == gc.split_cases(rng)
    assert [strip(c) for c in GOLDEN["correction"]] == json.loads(json.dumps(gc.correction_cases(rng)))
    assert [strip(c) for c in GOLDEN["graph"]] == gc.graph_cases(rng)
    assert [strip(c) for c in GOLDEN["iterative"]] == json.loads(json.dumps(gc.iterative_cases(rng)))


# ---------------------------------------------------------------- split (CPU only)
def test_split_equals_the_reference_as_it_behaves():
    cases = GOLDEN["split"]
    assert len(cases) >= 80 and {c["min_length"] for c in cases} >= set(range(1, 7))
    for case in cases:
        assert gc.run_split(MODS, case) == case["want"], case["read"]
    raised = [c for c in cases if "raises" in c["want"]]
    assert {c["want"]["raises"] for c in raised} >= {"IndexError"} and len(raised) >= 8
    by_text = {(c["read"][1], c["read"][2], c["min_length"]): c["want"] for c in cases}
    # the strings of DESIGN §29: DEF gets an EMPTY mono2nucl, DEFGH only its first letter
    assert by_text[("ABC?DEF", "+", 1)]["parts"][1][1:] == ["DEF", "+", []]
    assert by_text[("ABC?DEFGH", "+", 1)]["parts"][1][1:] == ["DEFGH", "+", [[0, "D", 400, 499]]]


# ---------------------------------------------------------------- the correction steps
@pytest.mark.parametrize("case", GOLDEN["correction"], ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_correction_steps_equal_the_reference(emu_session, case):
    assert gc.run_correction(MODS, case) == case["want"]


def test_the_correction_cases_cover_the_issues_list():
    names = " | ".join(c["name"] for c in GOLDEN["correction"])
    for what in ("share of exactly 0.1", "exactly max_gap", "shorter", "empty read", "exactly 0.05", "exactly min_length", "rotated", "two HORs", "nhor = 2",
                 "disqualifies the next", "share of exactly max_gap", "no frequent 3-mer", "whole"):
        assert what in names, what
    assert {c["step"] for c in GOLDEN["correction"]} == {"filter", "trim", "cut", "gaps", "whole"}
    # a fill happened, and one was refused
    gaps = [c for c in GOLDEN["correction"] if c["step"] == "gaps"]
    assert any(r_in[1].count("?") > r_out[1].count("?") > 0 for c in gaps for r_in, r_out in zip(c["reads"], c["want"]["reads"]))


# ---------------------------------------------------------------- the graph
@pytest.mark.parametrize("case", SMALL["graph"], ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_graph_cases_equal_the_reference(emu_session, case):
    got = gc.run_graph(MODS, case)
    for key in case["want"]:
        assert got[key] == case["want"][key], key
    assert set(got) == set(case["want"])


def test_the_graph_cases_cover_the_issues_list():
    names = " | ".join(c["name"] for c in GOLDEN["graph"])
    for what in ("pure cycle", "second component", "bubble", "complex node", "self-loop", "300 reads", "seeded set"):
        assert what in names, what
    by = {c["name"]: c["want"] for c in GOLDEN["graph"]}
    assert by["a cycle beside a second component: the cycle removes itself"]["contigs"] == ["XYZWV"]
    assert by["a pure cycle"]["contigs"] and by["a complex node with in- and out-degree 2"]["n_complex"] == 1
    assert by["a complex node with in- and out-degree 2"]["complex"] and by["long unique edges"]["long_edges"]


@pytest.mark.parametrize("case", SMALL["iterative"], ids=lambda c: c["name"][:40].replace(" ", "_"))
def test_iterative_graph_equals_the_reference(emu_session, case, tmp_path):
    got = gc.run_iterative(MODS, case, str(tmp_path))
    for key in case["want"]:
        assert got[key] == case["want"][key], key
    assert os.listdir(tmp_path) and not any(f.endswith(".dot") for d in os.listdir(tmp_path) for f in os.listdir(tmp_path / d))

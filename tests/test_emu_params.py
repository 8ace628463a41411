"""cf_set_param, cf_get_param, cf_param_name and Engine.knobs on the host emulator (tests/emu): host code, so no GPU test.

CHECKED is every knob with a check: its refusal, values it accepts (the bounds and the values its rule singles out) and values
it refuses (one beyond either bound, and the singled-out ones).  FLAGS are the knobs that take every value and store value != 0.
FRESH is what a fresh context holds.  All three are literals on purpose: they pin what callers see, whatever the library's
table (csrc/hip/cf_knobs.h) says."""
import os
import re

import pytest

from centroflye_amd.engine import DeviceError, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKED = {
    "dist_block": ("dist_block must be 0 (auto) or a multiple of 64 in [64, 1024]", [0, 64, 1024], [-1, 63, 96, 1025, 1088]),
    "dist_wgs": ("dist_wgs out of range (0 = auto, 1 .. 8)", [0, 8], [-1, 9]),
    "dist_slots": ("dist_slots out of range (0 = auto, 256 .. 19200: table + work lists must fit the 160 KiB LDS)", [0, 256, 19200], [-1, 255, 19201]),
    "dist_hot_cap": ("dist_hot_cap must be >= 0", [0, 2 ** 31 - 1], [-1]),
    "dist_hot_entries": ("dist_hot_entries out of range (-1 = always keep the list, 0 .. 2^31 - 1)", [-1, 2 ** 31 - 1], [-2, 2 ** 31]),
    "lut_shift": ("lut_shift out of range (-1 = by the set's size, 0 .. 3)", [-1, 3], [-2, 4]),
    "dist_regions": ("dist_regions must be 0 (auto), 1, 2, 4 or 8", [0, 1, 2, 4, 8], [-1, 3, 9, 16]),
    "dist_dbits": ("dist_dbits must be 0 (auto) or 5 .. 8", [0, 5, 8], [-1, 4, 9]),
    "dist_fill_pct": ("dist_fill_pct out of range (10 .. 90)", [10, 90], [9, 91]),
    "dist_edge_chunk": ("dist_edge_chunk out of range (0 = default, 1 .. 2^20)", [0, 2 ** 20], [-1, 2 ** 20 + 1]),
    "dist_sketch_bits": ("dist_sketch_bits must be 0 (by min_cov), 4 or 8", [0, 4, 8], [-1, 2, 9]),
    "dist_class_bits": ("dist_class_bits out of range (1 .. 16)", [1, 16], [0, 17]),
    "dist_group_cap": ("dist_group_cap out of range (1 .. 32)", [1, 32], [0, 33]),
    "dist_est_pct": ("dist_est_pct out of range (5 .. 100)", [5, 100], [4, 101]),
    "dist_stage": ("dist_stage out of range (0 .. 2048)", [0, 2048], [-1, 2049]),
    "place_mode": ("place_mode out of range (1 = hash map, 2 = per-read regions unless min_inters < 4, 3 = per-read regions always)", [1, 3], [0, 4]),
    "place_block": ("place_block must be 0 or a multiple of 128 in 128 .. 1024", [0, 128, 1024], [-1, 64, 127, 192, 1025, 1152]),
    "place_row_words": ("place_row_words must be 0 (auto), 32 or 64", [0, 32, 64], [-1, 16, 65]),
    "place_l3": ("place_l3 must be 0 (auto), 1 (always) or 2 (never)", [0, 2], [-1, 3]),
    "place_l3_shift": ("place_l3_shift must be 0 (= 6) .. 6", [0, 6], [-1, 7]),
    "place_long_rescans": ("place_long_rescans out of range (-1, 0 .. 1000000)", [-1, 1000000], [-2, 1000001]),
    "place_cmap_bits": ("place_cmap_bits out of range (0 = default, 1 .. 30)", [0, 30], [-1, 31]),
    "place_slots_per_unit": ("place_slots_per_unit out of range (0 = default, 1 .. 65536)", [0, 65536], [-1, 65537]),
    "place_chunk": ("place_chunk out of range (1 .. 64)", [1, 64], [0, 65]),
    "place_grid": ("place_grid out of range (0 = auto, 1 .. 4096)", [0, 4096], [-1, 4097]),
    "map_window": ("map_window out of range (0 = default, 1 .. 4096: 12 bytes of LDS per slot)", [0, 4096], [-1, 4097]),
    "edit_lds_diags": ("edit_lds_diags out of range (0 = default, 1 .. 16384: 8 bytes of LDS per diagonal)", [0, 16384], [-1, 16385]),
    "tandem_key_mode": ("tandem_key_mode out of range (0 = auto, 1 = 64-bit keys, 2 = 16-byte records)", [0, 2], [-1, 3]),
    "tandem_batch_windows": ("tandem_batch_windows out of range (0 = default, 1 .. 2^31)", [0, 2 ** 31], [-1, 2 ** 31 + 1]),
    "cons_batch_bytes": ("cons_batch_bytes out of range (0 = default, 1 .. 2^36)", [0, 2 ** 36], [-1, 2 ** 36 + 1]),
    "ualign_batch_bytes": ("ualign_batch_bytes out of range (0 = default, 1 .. 2^36)", [0, 2 ** 36], [-1, 2 ** 36 + 1]),
    "monodec_batch_bytes": ("monodec_batch_bytes out of range (0 = default, 1 .. 2^36)", [0, 2 ** 36], [-1, 2 ** 36 + 1]),
    "count_bits": ("count_bits out of range (0 = auto, 1 .. 27)", [0, 27], [-1, 28]),
    "count_slots": ("count_slots must be a power of two in [256, 16384]", [256, 16384], [128, 255, 384, 16385, 32768]),
    "count_tile": ("count_tile out of range", [1, 64], [0, 65]),
    "count_skip_exotic": ("count_skip_exotic must be 0 or 1", [0, 1], [-1, 2]),
    "comm_round_bytes": ("comm_round_bytes must be a multiple of 16 in [16, 2^30]", [16, 2 ** 30], [8, 15, 24, 2 ** 30 + 1, 2 ** 30 + 16]),
}
FLAGS = ("dist_wide", "dist_post_atomics", "dist_int_thr", "dist_sketch_tail", "dist_classes", "dist_groups", "dist_filter_once",
         "dist_sketch", "place_fused", "dist_region_bytes", "count_mode", "comm_self_p2p")
FRESH = dict(
    dist_block=0, dist_wgs=0, dist_slots=0, dist_wide=0, dist_post_atomics=0, dist_hot_cap=0, lut_shift=-1, dist_hot_entries=32768,
    dist_regions=0, dist_region_bytes=0, dist_dbits=0, dist_fill_pct=70, dist_edge_chunk=0, dist_int_thr=1, dist_sketch=1,
    dist_sketch_tail=1, dist_class_bits=16, dist_classes=1, dist_groups=1, dist_filter_once=1, dist_group_cap=32, dist_sketch_bits=0,
    dist_est_pct=80, dist_stage=2048, place_chunk=2, place_grid=0, place_fused=1, place_mode=2, place_block=0, place_row_words=0,
    place_long_rescans=2, place_cmap_bits=0, place_slots_per_unit=0, place_l3=0, place_l3_shift=0, map_window=0, edit_lds_diags=0,
    tandem_key_mode=0, tandem_batch_windows=0, cons_batch_bytes=0, ualign_batch_bytes=0, monodec_batch_bytes=0, count_mode=1,
    count_bits=0, count_slots=4096, count_tile=16, count_skip_exotic=0, comm_round_bytes=268435456, comm_self_p2p=0)


@pytest.fixture
def engine(emu_lib):
    with Engine(0, emu_lib) as e:
        yield e


def raw_set(engine, name, value):
    """(return code, message) of cf_set_param itself."""
    rc = engine._lib.cf_set_param(engine._ctx, name.encode(), value)
    return rc, engine._lib.cf_last_error(engine._ctx).decode()


# ---------------------------------------------------------------- cf_set_param alone (this part passes on the library before the table too)
def test_the_matrix_names_every_knob_once():
    assert len(CHECKED) == 37 and len(FLAGS) == 12 and not set(CHECKED) & set(FLAGS)
    assert set(CHECKED) | set(FLAGS) == set(FRESH)


@pytest.mark.parametrize("name", sorted(CHECKED))
def test_refusal_matrix(engine, name):
    message, accepted, refused = CHECKED[name]
    for v in accepted:
        assert raw_set(engine, name, v)[0] == 0, (name, v)
    for v in refused:
        assert raw_set(engine, name, v) == (-22, message), (name, v)
    assert raw_set(engine, name, accepted[0])[0] == 0       # a refusal does not stick


@pytest.mark.parametrize("name", FLAGS)
def test_flags_are_never_refused(engine, name):
    for v in (0, 1, 5, -3, 2 ** 62, -2 ** 63):
        assert raw_set(engine, name, v)[0] == 0, (name, v)


def test_set_refuses_an_unknown_name(engine):
    assert raw_set(engine, "dist_blok", 0) == (-22, "unknown parameter dist_blok")
    assert raw_set(engine, "", 0) == (-22, "unknown parameter ")
    with pytest.raises(DeviceError, match=r"cf_set_param\(no_such_knob\) failed \(-22\): unknown parameter no_such_knob"):
        engine.set_param("no_such_knob", 1)


# ---------------------------------------------------------------- cf_get_param, cf_param_name
def test_defaults_of_a_fresh_context(engine):
    names = engine.param_names()
    assert len(names) == 49 and len(set(names)) == 49
    assert {n: engine.get_param(n) for n in names} == FRESH


def test_param_name_ends_with_null(engine):
    lib = engine._lib
    assert lib.cf_param_name(-1) is None and lib.cf_param_name(49) is None and lib.cf_param_name(2 ** 31 - 1) is None
    assert lib.cf_param_name(0).decode() == engine.param_names()[0]


@pytest.mark.parametrize("name", sorted(CHECKED))
def test_accepted_values_read_back(engine, name):
    for v in CHECKED[name][1]:
        engine.set_param(name, v)
        assert engine.get_param(name) == v, (name, v)


@pytest.mark.parametrize("name", FLAGS)
def test_flags_read_back_as_0_or_1(engine, name):
    for v, want in ((0, 0), (1, 1), (5, 1), (0, 0), (-3, 1), (2 ** 62, 1)):
        engine.set_param(name, v)
        assert engine.get_param(name) == want, (name, v)


@pytest.mark.parametrize("name", sorted(CHECKED))
def test_a_refused_set_leaves_the_knob_unchanged(engine, name):
    _, accepted, refused = CHECKED[name]
    for before in (FRESH[name], accepted[-1]):
        engine.set_param(name, before)
        for v in refused:
            with pytest.raises(DeviceError):
                engine.set_param(name, v)
            assert engine.get_param(name) == before, (name, v)


def test_get_refuses_an_unknown_name_and_a_null_pointer(engine):
    with pytest.raises(DeviceError, match=r"cf_get_param\(dist_blok\) failed \(-22\): unknown parameter dist_blok"):
        engine.get_param("dist_blok")
    assert engine._lib.cf_get_param(engine._ctx, b"dist_block", None) == -22
    assert engine._lib.cf_get_param(engine._ctx, None, None) == -22


# ---------------------------------------------------------------- Engine.knobs
def test_knobs_restores_after_a_normal_body(engine):
    engine.set_param("dist_slots", 512)                      # not the default: what comes back is the value before, not the default
    with engine.knobs(dist_slots=2048, dist_sketch=0, count_tile=64) as e:
        assert e is engine
        assert [engine.get_param(n) for n in ("dist_slots", "dist_sketch", "count_tile")] == [2048, 0, 64]
    assert [engine.get_param(n) for n in ("dist_slots", "dist_sketch", "count_tile")] == [512, 1, 16]


def test_knobs_restores_after_a_raising_body(engine):
    with pytest.raises(KeyError):
        with engine.knobs(dist_block=128, dist_fill_pct=10):
            engine.set_param("dist_block", 256)              # a change inside the body goes too
            raise KeyError("body")
    assert engine.get_param("dist_block") == 0 and engine.get_param("dist_fill_pct") == 70


def test_knobs_restores_after_a_refused_second_setting(engine):
    entered = False
    with pytest.raises(DeviceError, match="dist_block must be 0"):
        with engine.knobs(dist_slots=256, dist_block=96, dist_sketch=0):
            entered = True
    assert not entered
    assert {n: engine.get_param(n) for n in FRESH} == FRESH
    with pytest.raises(DeviceError, match="unknown parameter dist_blok"):     # nothing is set when a name is unknown
        with engine.knobs(dist_slots=256, dist_blok=1):
            entered = True
    assert not entered and engine.get_param("dist_slots") == 0


def test_knobs_nest(engine):
    with engine.knobs(dist_slots=2048, dist_block=128):
        with engine.knobs(dist_slots=256, dist_sketch=0):
            assert [engine.get_param(n) for n in ("dist_slots", "dist_block", "dist_sketch")] == [256, 128, 0]
        assert [engine.get_param(n) for n in ("dist_slots", "dist_block", "dist_sketch")] == [2048, 128, 1]
    assert [engine.get_param(n) for n in ("dist_slots", "dist_block", "dist_sketch")] == [0, 0, 1]


def test_knobs_sets_in_the_order_given_and_restores_in_reverse(engine, monkeypatch):
    calls = []
    real = Engine.set_param
    monkeypatch.setattr(Engine, "set_param", lambda self, n, v: (calls.append((n, v)), real(self, n, v))[1])
    with engine.knobs(count_tile=1, dist_slots=256, count_mode=0):
        pass
    assert calls == [("count_tile", 1), ("dist_slots", 256), ("count_mode", 0), ("count_mode", 1), ("dist_slots", 0), ("count_tile", 16)]


# ---------------------------------------------------------------- the public header names the same knobs
def test_the_header_documents_exactly_the_knobs_of_the_library(engine):
    with open(os.path.join(ROOT, "include", "cfhip.h")) as f:
        text = f.read()
    doc = text[text.index("/* Tuning knobs"):text.index("int cf_set_param")]
    assert set(re.findall(r'"([a-z0-9_]+)"', doc)) == set(engine.param_names())

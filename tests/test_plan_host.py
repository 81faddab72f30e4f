"""The batch plan of the library (pngloss_amd/csrc/pl_plan.h: engine pin, row engine per image, launch groups, enumeration kind, runaway bound, host
window chunks) run on the CPU through tests/c/plan_host.cpp -- the same header pl_host.hip carries out.  Every expected value follows from the rules as
they stood before the plan was pulled out of pl_host.hip; the anchors are the ones the GPU suite asserts through engine_info
(test_gpu_parity.py: test_segment_engine_is_the_default_for_single_images_and_reports_what_it_did, test_engine_choice_on_batches_of_1080p_frames)."""
import numpy as np
import pytest

from tests import util as U

KNOBS = ["forced_filter", "rows_fit", "sync_call", "three_groups_ok", "launch_groups", "stream_wait_used", "seg_groups", "seg_unit", "tparts", "enum_nt", "kin",
         "seg_seeds", "seg_seeds1", "seed_kin", "force_careful", "segprof"]
DEFAULTS = dict(forced_filter=-1, rows_fit=1, sync_call=0, three_groups_ok=0, launch_groups=0, stream_wait_used=0, seg_groups=0, seg_unit=-1, tparts=0, enum_nt=0,
                kin=-1, seg_seeds=-1, seg_seeds1=-1, seed_kin=-1, force_careful=0, segprof=0)
SEG_ALL, SEG_SEEDS, UNITS_ALL, UNITS_SEEDS, SEEDED = range(5)      # PlEnumKind
HD = (1920, 1080)


def plan(sizes, s=19, b=2, engine=None, cus=256.0, seg=1.0, wg=1.0, **knobs):
    """pl_plan_batch for images of (width, height); engine: the value of $PNGLOSS_HIP_ENGINE (None: unset)"""
    lib = U.plan_host_lib()
    n = len(sizes)
    w = np.array([x[0] for x in sizes] or [0], np.uint32)
    h = np.array([x[1] for x in sizes] or [0], np.uint32)
    k = dict(DEFAULTS)
    assert set(knobs) <= set(k), knobs
    k.update(knobs)
    kv = np.array([int(k[x]) for x in KNOBS], np.int32)
    sc = np.array([cus, seg, wg], np.float64)
    out = np.zeros(16, np.int64)
    on = np.zeros(max(n, 1), np.uint8)
    sl = np.zeros(max(n, 1), np.uint32)
    g = np.zeros(8 * 12, np.int64)
    lib.plan_host_run(w.ctypes.data, h.ctypes.data, n, s, b, None if engine is None else engine.encode(), kv.ctypes.data, sc.ctypes.data, out.ctypes.data,
                      on.ctypes.data, sl.ctypes.data, g.ctypes.data)
    groups = [dict(zip(["first", "n", "max_nseg", "max_ngrp", "max_ncommit", "enum_nt", "tparts", "unit", "seeds", "small_ok", "seeded"], map(int, row[:11])))
              for row in g.reshape(8, 12)[:int(out[5])]]
    return dict(use_rows=bool(out[0]), seg_costed=bool(out[1]), seg_pin_unmet=bool(out[2]), engine_mode=int(out[3]), kind=int(out[4]), ngroups=int(out[5]),
                unit=int(out[6]), tparts=int(out[7]), seed_kin=int(out[8]), kin=int(out[9]), max_attempts=int(out[10]), engine_flags=int(out[12]),
                seeded=bool(out[13]), on_seg=[int(x) for x in on[:n]], seg_list=[int(x) for x in sl[:int(out[11])]], groups=groups)


def all_seg(p):
    return len(p["on_seg"]) > 0 and all(p["on_seg"])


def none_seg(p):
    return not any(p["on_seg"])


# ---- which row engine ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,s,b,on_seg", [(1000, 19, 2, 1), (1000, 85, 2, 1), (1000, 255, 1, 1), (200, 19, 2, 0)])
def test_single_images_wide_to_the_segment_engine_narrow_to_the_workgroup_engine(w, s, b, on_seg):
    p = plan([(w, 70)], s, b)
    assert p["on_seg"] == [on_seg] and p["seg_costed"] and not p["use_rows"]
    if on_seg:
        assert p["ngroups"] == 1 and p["kind"] == (SEG_ALL if s == 19 else SEEDED)


def test_1080p_batches_either_side_of_the_crossover():
    assert all_seg(plan([HD] * 136))
    assert none_seg(plan([HD] * 164))
    assert none_seg(plan([HD] * 137))          # (the first batch past the segment engine's 8192 segments)


def _crossover(size, **kw):
    """the smallest batch of `size` frames that the cost model gives wholly to the workgroup engine"""
    for n in range(1, 600):
        if none_seg(plan([size] * n, **kw)):
            return n
    raise AssertionError("no crossover")


def test_crossover_moves_with_the_cu_count_and_the_calibration_scales():
    base = _crossover(HD)
    assert base == 137
    # a machine with fewer CUs, a slower segment engine or a faster workgroup engine: fewer 1080p frames on the segment engine
    for kw, want in [(dict(cus=128.0), 75), (dict(cus=200.0), 117), (dict(seg=1.2), 122), (dict(wg=0.8), 117)]:
        assert _crossover(HD, **kw) == want, kw
        assert not all_seg(plan([HD] * 136, **kw)), kw
    # ... the other way the 1080p batch is held at 136 frames by the segment engine's 8192 segments; 1280x720 frames show the move
    for kw in [dict(cus=304.0), dict(seg=0.8), dict(wg=1.2)]:
        assert _crossover(HD, **kw) == base, kw
    hd720 = (1280, 720)
    b720 = _crossover(hd720)
    assert b720 == 130
    for kw, want in [(dict(cus=128.0), 65), (dict(cus=304.0), 154), (dict(seg=1.2), 104), (dict(seg=0.8), 168), (dict(wg=1.2), 160), (dict(wg=0.8), 99)]:
        assert _crossover(hd720, **kw) == want, kw


def test_strength_0_uses_the_row_statistics_engine_unless_pinned_or_short_of_memory():
    batch = [(640, 48), (1000, 70)]
    assert plan(batch, 0)["use_rows"] and none_seg(plan(batch, 0))
    assert plan(batch, 0, engine="rows")["use_rows"]
    assert plan(batch, 0, engine="auto")["use_rows"]
    assert plan(batch, 0, engine="")["use_rows"]
    for kw in [dict(rows_fit=0), dict(force_careful=1), dict(forced_filter=0), dict(engine="seg"), dict(engine="wg"), dict(engine="lead"), dict(engine="mix")]:
        assert not plan(batch, 0, **kw)["use_rows"], kw
    p = plan(batch, 0, rows_fit=0)          # (the long way: the cost model as at any other strength)
    assert p["seg_costed"] and p["on_seg"] == [1, 1]
    assert not plan(batch, 0, force_careful=1)["seg_costed"] and none_seg(plan(batch, 0, force_careful=1))
    for engine in [None, "rows", "auto"]:
        assert not plan(batch, 1, engine=engine)["use_rows"], engine


@pytest.mark.parametrize("engine,mode,split", [
    (None, 0, [1, 0]), ("auto", 0, [1, 0]), ("", 0, [1, 0]), ("rows", 0, [1, 0]), ("seg", 0, [1, 1]), ("wg", 0, [0, 0]), ("lead", 2, [0, 0]),
    ("legacy", 1, [0, 0]), ("mix", 3, [0, 0]), ("bogus", 0, [0, 0])])
def test_engine_pins(engine, mode, split):
    p = plan([(1000, 70)], 19, 2, engine=engine)
    q = plan([(200, 70)], 19, 2, engine=engine)
    assert p["engine_mode"] == mode and q["engine_mode"] == mode and p["on_seg"] + q["on_seg"] == split and not p["use_rows"]
    assert p["seg_costed"] == (engine in (None, "", "auto", "rows"))
    assert not p["seg_pin_unmet"]


def test_seg_pin_with_nothing_the_segment_engine_takes():
    p = plan([(0, 5), ((1 << 20) + 1, 2), (7, 0)], engine="seg")
    assert p["seg_pin_unmet"] and none_seg(p) and p["ngroups"] == 0
    assert not plan([], engine="seg")["seg_pin_unmet"]
    assert plan([(1 << 20, 2), ((1 << 20) + 1, 2)], engine="seg")["on_seg"] == [1, 0]


def test_forced_filter_build():
    p = plan([(1000, 70)], 19, 2, forced_filter=3, segprof=1)
    assert p["engine_mode"] == 4 << 8 and p["engine_flags"] == (4 << 8) | 1
    assert plan([(1000, 70)], 19, 2, engine="mix", forced_filter=0)["engine_mode"] == 3 | (1 << 8)
    assert plan([(1000, 70)], 19, 2)["engine_flags"] == 0 and plan([(1000, 70)], 19, 2, segprof=1)["engine_flags"] == 1


def test_engine_option_names():
    lib = U.plan_host_lib()
    for i, name in enumerate(["auto", "seg", "wg", "lead", "legacy", "mix", "rows"]):
        assert lib.plan_host_parse_option(name.encode()) == i
    for bad in ["", "bogus", "Seg", "auto "]:
        assert lib.plan_host_parse_option(bad.encode()) == -1


# ---- launch groups -------------------------------------------------------------------------------------------------------------------------------------------

STRIPS = [(1920, 40)] * 14            # 840 segments: more than SEG_UNIT_MIN_SEGS, and eight images or more


def test_launch_groups_of_a_batch_of_strips():
    p = plan(STRIPS)
    assert all_seg(p) and p["ngroups"] == 2 and [g["n"] for g in p["groups"]] == [7, 7]
    three = dict(launch_groups=3, sync_call=1, three_groups_ok=1)
    p = plan(STRIPS, **three)
    assert p["ngroups"] == 3 and [g["first"] for g in p["groups"]] == [0, 4, 9] and [g["n"] for g in p["groups"]] == [4, 5, 5]
    for off in ["launch_groups", "sync_call", "three_groups_ok"]:
        assert plan(STRIPS, **dict(three, **{off: 0}))["ngroups"] == 2, off
    assert plan(STRIPS, stream_wait_used=1, **three)["ngroups"] == 2
    assert plan(STRIPS[:11], engine="seg", **three)["ngroups"] == 2          # (three from twelve images on)
    assert plan(STRIPS, seg_groups=1)["ngroups"] == 1
    assert plan(STRIPS, seg_groups=5)["ngroups"] == 5
    assert plan(STRIPS[:3], engine="seg", seg_groups=5)["ngroups"] == 3


def test_launch_groups_tallest_image_alone_when_it_stands_out():
    p = plan([(300, 40), (200, 90), (64, 48), (700, 25), (33, 77), (1, 1), (512, 90)], engine="seg")      # tallest in the middle, a tie for the tallest
    assert p["seg_list"] == [1, 6, 4, 2, 0, 3, 5] and p["ngroups"] == 2 and [g["first"] for g in p["groups"]] == [0, 3]
    p = plan([(96, 120), (400, 16), (300, 16), (50, 16)], engine="seg")
    assert p["seg_list"] == [0, 1, 2, 3] and [g["first"] for g in p["groups"]] == [0, 1] and [g["n"] for g in p["groups"]] == [1, 3]
    assert [g["first"] for g in plan([(96, 105), (400, 100), (300, 16), (50, 16)], engine="seg")["groups"]] == [0, 2]    # 5 %: not beyond
    assert [g["first"] for g in plan([(96, 106), (400, 100), (300, 16), (50, 16)], engine="seg")["groups"]] == [0, 1]
    assert [g["n"] for g in plan([(96, 120), (400, 16), (300, 16), (50, 16)], engine="seg", seg_groups=2)["groups"]] == [2, 2]   # (the hook: equal shares)
    assert plan([(260, 30), (180, 64)], engine="seg")["ngroups"] == 2


def test_launch_groups_with_an_empty_and_a_one_pixel_image():
    p = plan([(0, 50), (1, 1), (640, 20), (640, 20)], engine="seg")
    assert p["on_seg"] == [0, 1, 1, 1] and p["seg_list"] == [2, 3, 1] and p["ngroups"] == 2
    assert [(g["first"], g["n"]) for g in p["groups"]] == [(0, 1), (1, 2)]
    assert [(g["max_nseg"], g["max_ngrp"], g["max_ncommit"]) for g in p["groups"]] == [(20, 2, 3), (20, 2, 3)]
    p = plan([(1, 1)], engine="seg")
    assert p["ngroups"] == 1 and p["groups"][0]["max_nseg"] == 1 and p["groups"][0]["max_ncommit"] == 1 and p["groups"][0]["enum_nt"] == 512


# ---- enumeration kind ----------------------------------------------------------------------------------------------------------------------------------------

def kind(segs, k, s=19, b=2, seg_unit=-1, seg_seeds=-1, seg_seeds1=-1):
    return U.plan_host_lib().plan_host_enum_kind(segs, k, s, b, seg_unit, seg_seeds, seg_seeds1)


def test_pairs_with_and_without_a_seed_set():
    lib = U.plan_host_lib()
    assert lib.plan_host_seed_n(19, 2) > 0 and lib.plan_host_seed_n(20, 2) == 0
    assert lib.plan_host_seed_n(30, 8) == 0
    assert kind(10, 1, 85, 1) == SEEDED and kind(10, 1, 20, 2) == SEG_ALL and kind(5000, 20, 20, 2) == SEG_ALL      # (20, 2): more states than a chunk of lanes


@pytest.mark.parametrize("segs,k,want", [
    (329, 2, SEG_ALL), (330, 2, SEG_SEEDS),                      # SEG_SEEDS1_MIN_SEGS
    (351, 11, SEG_ALL), (352, 11, SEG_SEEDS),                    # SEG_SEEDS1_MIN_SEGS_PER_IMAGE
    (400, 1, SEG_ALL), (680, 1, SEG_ALL), (681, 1, UNITS_SEEDS),  # one image: never segment by segment from seeds; SEG_UNIT_MIN_SEGS
    (680, 30, SEG_ALL), (681, 30, UNITS_SEEDS),                  # SEG_UNIT_MIN_SEGS (fewer than 32 segments an image)
    (1000, 2, SEG_SEEDS), (1001, 2, UNITS_SEEDS),                # SEG_UNIT_MIN_SEGS_SEEDS
])
def test_enumeration_kind_thresholds_with_a_seed_set(segs, k, want):
    assert kind(segs, k) == want


@pytest.mark.parametrize("segs,k,want", [(330, 2, SEG_ALL), (680, 2, SEG_ALL), (681, 2, UNITS_ALL), (1001, 2, UNITS_ALL), (681, 1, UNITS_ALL)])
def test_enumeration_kind_thresholds_without_a_seed_set(segs, k, want):
    assert kind(segs, k, 30, 8) == want
    assert kind(segs, k, 19, 2, seg_seeds=0) == want


def test_enumeration_kind_pins():
    assert kind(10, 1, seg_unit=1) == UNITS_SEEDS and kind(10, 1, 30, 8, seg_unit=1) == UNITS_ALL and kind(10, 1, 20, 2, seg_unit=1) == SEG_ALL
    assert kind(5000, 2, seg_unit=0) == SEG_SEEDS and kind(5000, 1, seg_unit=0) == SEG_ALL
    assert kind(10, 1, seg_seeds1=1) == SEG_SEEDS and kind(330, 2, seg_seeds1=0) == SEG_ALL
    assert kind(5000, 2, seg_seeds1=0) == UNITS_SEEDS and kind(10, 1, 30, 8, seg_seeds1=1) == SEG_ALL
    assert kind(330, 2, seg_seeds=0, seg_seeds1=1) == SEG_ALL
    assert kind(10, 1, seg_seeds=1) == SEG_ALL and kind(330, 2, seg_seeds=1) == SEG_SEEDS
    for pins in [dict(seg_unit=1), dict(seg_unit=0), dict(seg_seeds1=1), dict(seg_seeds=0)]:
        assert kind(5000, 20, 85, 1, **pins) == SEEDED, pins


def test_the_plan_carries_the_kind_into_the_groups():
    units = [(1920, 40)] * 24                              # 1440 segments: in units, from seeds
    p = plan(units)
    assert p["kind"] == UNITS_SEEDS and p["unit"] == 3 and p["tparts"] == 1
    assert all(g["unit"] == 3 and g["tparts"] == 1 and g["seeds"] and g["enum_nt"] == 1024 for g in p["groups"])
    p = plan(STRIPS)                                       # 840 segments, 60 an image: segment by segment from seeds, up to SEG_UNIT_MIN_SEGS_SEEDS
    assert p["kind"] == SEG_SEEDS and p["unit"] == 1 and p["tparts"] == 4 and all(g["seeds"] and g["unit"] == 1 for g in p["groups"])
    p = plan([(1536, 20)] * 8)                             # 384 segments: segment by segment from seeds (smoke()'s batch)
    assert all_seg(p) and p["kind"] == SEG_SEEDS and p["unit"] == 1 and p["tparts"] == 4 and all(g["seeds"] for g in p["groups"])
    p = plan([(1536, 20)] * 8, seg_seeds1=0)
    assert p["kind"] == SEG_ALL and not any(g["seeds"] for g in p["groups"])
    p = plan(units, seg_unit=0)
    assert p["kind"] == SEG_SEEDS and p["unit"] == 1 and p["tparts"] == 4
    p = plan(STRIPS, seg_unit=1)
    assert p["kind"] == UNITS_SEEDS and p["unit"] == 3 and p["tparts"] == 1
    p = plan(STRIPS, seg_seeds=0)
    assert p["kind"] == UNITS_ALL and p["unit"] == 3 and not any(g["seeds"] for g in p["groups"])
    p = plan(units, tparts=4)
    assert p["unit"] == 3 and p["tparts"] == 4 and all(g["tparts"] == 4 for g in p["groups"])
    assert plan([(1000, 70)], tparts=1)["tparts"] == 1 and plan([(1000, 70)], tparts=2)["tparts"] == 4
    p = plan([(1000, 70)], 85, 1)
    assert p["kind"] == SEEDED and p["seeded"] and p["unit"] == 1 and p["groups"][0]["seeded"] and not p["groups"][0]["seeds"] and not p["groups"][0]["small_ok"]
    assert plan([(1000, 70)], 85, 1, kin=30)["kin"] == 30 and plan([(1000, 70)], 85, 1, kin=33)["kin"] == p["kin"] and plan([(1000, 70)], 19, 2, kin=30)["kin"] == 0
    assert plan(STRIPS, seed_kin=5)["seed_kin"] == 5 and plan(STRIPS, seed_kin=17)["seed_kin"] == plan(STRIPS)["seed_kin"]


def test_enumeration_workgroup_size():
    # SEG_ENUM_NT_SMALL_MAX_NSEG = 320 segments in a launch group: 512 threads up to there, 1024 beyond
    assert plan([(320 * 32, 4)], engine="seg")["groups"][0]["enum_nt"] == 512
    assert plan([(320 * 32 + 1, 4)], engine="seg")["groups"][0]["enum_nt"] == 1024
    p = plan([(1920, 30)] * 10 + [(1920, 20)] * 10, engine="seg", seg_groups=2)      # 600 segments a group
    assert [g["enum_nt"] for g in p["groups"]] == [1024, 1024]
    p = plan([(1920, 30)] * 5 + [(1920, 20)] * 5, engine="seg", seg_groups=2)        # 300
    assert [g["enum_nt"] for g in p["groups"]] == [512, 512]
    assert plan([(1920, 30)] * 5, engine="seg", enum_nt=1024)["groups"][0]["enum_nt"] == 1024
    assert plan([(320 * 32 + 1, 4)], engine="seg", enum_nt=512)["groups"][0]["enum_nt"] == 512
    assert plan([(320 * 32 + 1, 4)], engine="seg", enum_nt=700)["groups"][0]["enum_nt"] == 1024


def test_runaway_bound():
    # rows of the tallest image x (strength + 1) x (2 + 2 x SEG_MAX_RESTARTS x 5) + 1024
    assert plan([(1000, 70)], 19, 2)["max_attempts"] == 70 * 20 * 122 + 1024
    assert plan([(300, 40), (200, 90), (1, 1)], 0, 2, engine="seg")["max_attempts"] == 90 * 1 * 122 + 1024
    assert plan([(1000, 1 << 20)], 255, 1, engine="seg")["max_attempts"] == 2000000000


# ---- host window ---------------------------------------------------------------------------------------------------------------------------------------------

def window(pixels, split=0, no_split=0, deflate=0, peers=8):
    first = np.zeros(9, np.uint64)
    px = np.array(pixels or [0], np.uint64)
    K = U.plan_host_lib().plan_host_window(px.ctypes.data, len(pixels), split, no_split, deflate, peers, first.ctypes.data)
    return [int(x) for x in first[:K + 1]]


def test_host_window_chunks():
    assert window([100]) == [0, 1]
    assert window([100] * 15) == [0, 15]
    assert window([100] * 16) == [0, 8, 16]
    assert window([1500] + [100] * 15) == [0, 1, 16]
    assert window([100] * 15 + [1500]) == [0, 15, 16]
    assert window([10, 20, 30, 40] * 4) == [0, 8, 16]
    assert window([100] * 16, split=4) == [0, 4, 8, 12, 16]
    assert window([100] * 3, split=4) == [0, 1, 2, 3]
    assert window([100] * 15, split=2) == [0, 8, 15]
    assert window([100] * 16, split=1) == [0, 16]
    assert window([100] * 16, no_split=1) == [0, 16]
    assert window([100] * 16, split=4, no_split=1) == [0, 16]
    assert window([100] * 16, deflate=1) == [0, 16]
    assert window([100] * 16, split=4, peers=1) == [0, 8, 16]
    assert window([100] * 16, peers=0) == [0, 16]
    assert window([0] * 16) == [0, 1, 16]
    assert window([1500] * 2 + [0] * 14, split=4) == [0, 1, 2, 3, 16]

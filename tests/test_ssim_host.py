"""CPU tests of the SSIM measurement (no GPU compute): the arithmetic of pngloss_amd/csrc/pl_ssim_core.h -- the two thread loops the kernel pl_ssim
runs per tile -- on the CPU under the sanitizers (tests/c/ssim_host.cpp) against the definition restated in Python integers and against the
textbook float formula (tests/util_ssim.py), tile by tile and as the kernel's workgroups take them, over a table that is never cleared; the launch
shape (pls_grid_blocks) against its restatement; pngloss_hip_ssim_mean on hand-made records; the check of a pngloss_hip_target2, the acceptance rule
with the SSIM condition and the arena layout (tests/c/target2_host.cpp); the exported symbols and the command line switches where no device is
needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_ssim as S
from tests import util_target as T
from tests import util_visible as V

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists("/opt/conda/include/png.h") or os.path.exists("/usr/include/png.h")
needs_cli = pytest.mark.skipif(not have_png, reason="libpng headers not found on this box: the command line tool is not built")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("ssim_host")
    return S.build_ssim_host(d), d


@pytest.fixture(scope="module")
def target2(tmp_path_factory):
    d = tmp_path_factory.mktemp("target2_host")
    return S.build_target2_host(d), d


def test_core_equals_the_definition_on_every_shape_and_content(harness):
    exe, d = harness
    cases = S.all_cases()
    got = S.run_ssim_host(exe, d, [(a, b, 0, 0, 256) for _, a, b in cases])
    assert {n.split("_")[0] for n, _, _ in cases} == {"%dx%d" % s for s in S.SHAPES}
    for (name, a, b), rec in zip(cases, got):
        want = S.expected(name)
        print(name, rec)
        assert rec == want, name
        assert rec["windows"] == S.geometry(a.shape[1], a.shape[0])[0] * S.geometry(a.shape[1], a.shape[0])[1] and rec["reserved"] == 0
        if rec["windows"] == 0:
            assert rec["sum_q16"] == [0] * 4 and rec["min_q16"] == [S.ONE] * 4
    by = {n: r for (n, _, _), r in zip(cases, got)}
    assert [by["%dx%d_equal" % s]["windows"] for s in S.SHAPES] == [1, 1, 4, 0, 0, 0, 2, 31 * 16, 74 * 18, 0]
    for w, h in S.SHAPES:
        n = by["%dx%d_equal" % (w, h)]["windows"]
        # equal pairs: every q is 65536 and the mean exactly 1.0; a checkerboard against its inverse: q = -65300 in every window (the sign rule)
        assert by["%dx%d_equal" % (w, h)]["sum_q16"] == [S.ONE * n] * 4 and by["%dx%d_equal" % (w, h)]["min_q16"] == [S.ONE] * 4
        assert by["%dx%d_checkerboard_inverse" % (w, h)]["sum_q16"] == [-65300 * n] * 4
        if n:
            assert P.ssim_mean(by["%dx%d_equal" % (w, h)], 0xF) == 1.0
            assert by["%dx%d_checkerboard_inverse" % (w, h)]["min_q16"] == [-65300] * 4


def test_mean_is_within_one_q16_step_of_the_float_formula():
    """the truncation of q loses less than 2^-16 per window; the rest is double rounding"""
    for name, a, b in S.all_cases():
        rec = S.expected(name)
        for mask in (0xF, 0x7, 0xA, 0x2):
            if rec["windows"]:
                m, f = P.ssim_mean(rec, mask), S.float_ssim(a, b, mask)
                assert m == S.py_mean(rec, mask)
                assert abs(m - f) <= 2.0 ** -16 + 1e-9, (name, mask, m, f)
            else:
                assert math.isnan(P.ssim_mean(rec, mask)) and math.isnan(S.float_ssim(a, b, mask))


def test_misaligned_bases_thread_counts_and_odd_pitches(harness):
    """bases 4, 8 and 12 bytes off a 16-byte boundary (word loads instead of 16-byte ones), few and many threads; the blocks end with the last pixel"""
    exe, d = harness
    picked = [c for c in S.all_cases() if c[0].split("_", 1)[1] in ("noise", "oracle") and c[0].split("_")[0] in ("12x12", "13x9", "131x69", "300x77")]
    assert len(picked) == 8
    cases, names = [], []
    for name, a, b in picked:
        for oa, ob in ((4, 0), (0, 8), (12, 12), (8, 4)):
            cases.append((a, b, oa, ob, 256)); names.append(name)
        for nt in (4, 64, 1024):
            cases.append((a, b, 0, 0, nt)); names.append(name)
    got = S.run_ssim_host(exe, d, cases)
    for name, rec in zip(names, got):
        assert rec == S.expected(name), name


def test_grid_rule_equals_its_restatement_at_the_pinned_points(harness):
    """pls_grid_blocks and PLS_MAX_IMAGES of pl_ssim_core.h -- what pl_ssim.hip launches with -- against S.grid_blocks, whose values at the pinned points
    are written out in S.GRID_POINTS"""
    exe, _ = harness
    assert S.GRID_N == [1, 5, 59, 255, 256, 257, 300, 65535] and sorted(S.GRID_POINTS) == [0, 1, 8, 9, 288, 4096]
    points = [(n, t) for t in sorted(S.GRID_POINTS) for n in S.GRID_N]
    points += [(n, t) for n in (2, 7, 8, 228, 229, 260, 2048, 2049, 65540) for t in (2, 7, 10, 20, 32, 297, 2047, 2048, 2049, 1 << 40)]
    max_images, got = S.run_ssim_grid(exe, points)
    assert max_images == S.MAX_IMAGES == 65535
    assert got == [S.grid_blocks(n, t) for n, t in points]
    assert got[: 6 * 8] == [b for t in sorted(S.GRID_POINTS) for b in S.GRID_POINTS[t]]
    # what the GPU tests rely on: 260 pairs put 8 workgroups on every image, 5 pairs one on (nearly) every tile
    assert S.grid_blocks(260, 297) == 8 and S.grid_blocks(5, 297) == 297 and S.grid_blocks(65535, 1) == S.grid_blocks(5, 1) == 1


#: (name of the pair, workgroups): 300x77, where tile 8 -- the 10 x 2-window corner -- follows the full tile 0 in workgroup 0; 5 x 4 tiles partial in
#: both directions, 3 and 2 trips; 32 full tiles on an odd width, 4 trips each; 2 x 2 tiles, all in one workgroup
WORKGROUP_CASES = [("300x77_noise", 8), ("643x131_near", 8), ("517x261_near", 8), ("136x40", 1)]


def test_a_workgroups_tiles_over_one_table_that_is_never_cleared(harness):
    """what LDS sees on the device: the table is poisoned once per workgroup, then the workgroup's tiles run over it one after the other, each leaving
    its cells behind for the next -- in both instantiations; the records are the definition's and those of the tile-by-tile run"""
    exe, d = harness
    plain = {n: (a, b) for n, a, b in S.trip_pairs()}
    plain["136x40"] = V.ssim_pairs()["136x40"]
    visible = {n: (a, b) for n, a, b in V.trip_pairs()}
    visible["136x40"] = V.ssim_pairs()["136x40"]
    cases, wants = [], []
    for name, blocks in WORKGROUP_CASES:
        for vis, pairs, ssim in ((0, plain, S.py_ssim), (1, visible, V.py_ssim)):
            a, b = pairs[name]
            per = S.trips(1, [(a.shape[1], a.shape[0])], a.shape[1], a.shape[0])
            assert len(per) == S.tiles_of(a.shape[1], a.shape[0]) > blocks           # (alone in a call every tile has a workgroup: the older tests)
            cases += [(a, b, 0, 0, 256, blocks, vis), (a, b, 0, 0, 256, 0, vis)]
            wants.append((name, vis, ssim(a, b)))
    assert [S.tiles_of(*plain[n][0].shape[1::-1]) for n, _ in WORKGROUP_CASES] == [9, 20, 32, 4]
    got = S.run_ssim_host(exe, d, cases)
    for k, (name, vis, want) in enumerate(wants):
        assert got[2 * k] == want and got[2 * k + 1] == want, (name, vis)
        assert want["windows"] > 0
    # the visible pairs drop windows, so the two instantiations were told apart
    assert all(wants[2 * k][2] != wants[2 * k + 1][2] for k in range(len(WORKGROUP_CASES)))


def test_closed_forms_of_the_two_uniform_pairs_equal_the_definition():
    """the GPU tests expect 66 048 x (-65300) and 66 049 x 65536 -- past -2^32 and 2^32 -- of the checkerboard and the equal pair: here the definition
    says so on the whole images"""
    got = {n: (a, b, S.py_ssim(a, b)) for n, a, b in S.trip_pairs() if n in ("1036x1028_checkerboard_inverse", "1032x1032_equal")}
    want = dict(zip([n for n, _, _ in S.trip_pairs()], S.trip_expected()))
    a, b, rec = got["1036x1028_checkerboard_inverse"]
    assert rec == want["1036x1028_checkerboard_inverse"] == S.uniform_record(a, b)
    assert rec == dict(windows=258 * 256, sum_q16=[66048 * -65300] * 4, min_q16=[-65300] * 4, reserved=0) and 66048 * -65300 == -4312934400 < -(1 << 32)
    a, b, rec = got["1032x1032_equal"]
    assert rec == want["1032x1032_equal"] == S.uniform_record(a, b)
    assert rec == dict(windows=257 * 257, sum_q16=[66049 * 65536] * 4, min_q16=[65536] * 4, reserved=0) and 66049 * 65536 > 1 << 32
    assert P.ssim_mean(rec, 0xF) == 1.0


def test_ssim_mean_on_hand_made_records_needs_no_device():
    rec = dict(windows=3, sum_q16=[3 * 65536, 0, -3 * 65536, 98304], min_q16=[65536, 0, -65536, 0])
    assert P.ssim_mean(rec, 0x1) == 1.0 and P.ssim_mean(rec, 0x2) == 0.0 and P.ssim_mean(rec, 0x4) == -1.0 and P.ssim_mean(rec, 0x8) == 0.5
    assert P.ssim_mean(rec, 0xF) == (3 * 65536 + 98304 - 3 * 65536) / (65536.0 * 3 * 4) == S.py_mean(rec, 0xF)
    assert P.Ssim(3, (C.c_int64 * 4)(*rec["sum_q16"]), (C.c_int32 * 4)(*rec["min_q16"]), 0).mean(0x8) == 0.5
    for mask in (0, 0x10, 0xFF):
        assert math.isnan(P.ssim_mean(rec, mask))
    assert math.isnan(P.ssim_mean(dict(rec, windows=0), 0xF))
    lib = P.hip_lib()
    assert math.isnan(lib.pngloss_hip_ssim_mean(None, 0xF))
    assert C.sizeof(P.Ssim) == 64 and P.Ssim.min_q16.offset == 40 and P.Ssim.reserved.offset == 56


def _accept_cmd(psnr, max_abs, ssim, status, bpp, pixels, sq, mx, windows, sums):
    return "A %s %d %s %d %d %d %s %s %d %s" % (T.double_bits(psnr), max_abs, T.double_bits(ssim), status, bpp, pixels, " ".join(map(str, sq)), " ".join(map(str, mx)),
                                                 windows, " ".join(map(str, sums)))


def test_target2_check_acceptance_and_layout(target2):
    exe, d = target2
    bad = [(35.0, 0, 19, math.nan), (35.0, 0, 19, -0.5), (35.0, 0, 19, 1.5), (35.0, 0, 19, math.inf), (math.nan, 0, 19, 0.5), (35.0, 256, 19, 0.5), (35.0, 0, 256, 0.5)]
    good = [(0.0, 0, 0, 0.0), (35.0, 0, 19, 0.0), (35.0, 8, 40, 1.0), (0.0, 0, 40, 0.95), (math.inf, 255, 255, 5e-324)]
    got = S.run_target2_host(exe, d, ["C %s %d %d %s" % (T.double_bits(p), e, m, T.double_bits(s)) for p, e, m, s in bad + good])
    assert got == [str(L.PNGLOSS_INVALID_ARGUMENT)] * len(bad) + ["0"] * len(good)
    # acceptance: 10 windows; a mean of exactly 0.75 over the stored channels of each class, 1.0 elsewhere
    cases = []
    full, part = 10 * 65536, 10 * 49152
    for bpp, mask in ((1, 0x2), (2, 0xA), (3, 0x7), (4, 0xF)):
        sums = [part if mask >> c & 1 else full for c in range(4)]
        inverse = [full if mask >> c & 1 else -full for c in range(4)]         # only channels outside the mask are bad
        for ssim, want in ((0.0, True), (0.75, True), (0.7500001, False), (1.0, False)):
            cases.append((want, _accept_cmd(0.0, 0, ssim, 0, bpp, 100, [0] * 4, [0] * 4, 10, sums)))
        cases.append((True, _accept_cmd(0.0, 0, 1.0, 0, bpp, 100, [0] * 4, [0] * 4, 10, inverse)))
        cases.append((True, _accept_cmd(0.0, 0, 1.0, 0, bpp, 35, [0] * 4, [0] * 4, 0, [0] * 4)))      # no window: cannot be measured, passes 1.0
        cases.append((False, _accept_cmd(0.0, 0, 0.5, 65, bpp, 100, [0] * 4, [0] * 4, 10, sums)))     # status not 0
        cases.append((False, _accept_cmd(0.0, 4, 0.5, 0, bpp, 100, [2500] * 4, [5] * 4, 10, sums)))   # the other conditions still hold: max_abs_error decides
        cases.append((False, _accept_cmd(60.0, 0, 0.5, 0, bpp, 100, [2500] * 4, [5] * 4, 10, sums)))  # ... and the PSNR
        cases.append((True, _accept_cmd(30.0, 5, 0.5, 0, bpp, 100, [2500] * 4, [5] * 4, 10, sums)))
    cases.append((True, _accept_cmd(0.0, 0, 1.0, 0, 4, 0, [0] * 4, [0] * 4, 0, [0] * 4)))             # an image without pixels
    got = S.run_target2_host(exe, d, [c for _, c in cases])
    for (want, cmd), line in zip(cases, got):
        assert line == ("1" if want else "0"), cmd
        f = cmd.split()                                  # and the Python restatement the other tests rely on agrees
        rec = dict(pixels=int(f[6]), changed_pixels=1, sq_err=[int(x) for x in f[7:11]], max_abs=[int(x) for x in f[11:15]])
        srec = dict(windows=int(f[15]), sum_q16=[int(x) for x in f[16:20]])
        unbits = lambda h: np.array([int(h, 16)], np.uint64).view(np.float64)[0]
        assert S.py_accept2(unbits(f[1]), int(f[2]), unbits(f[3]), rec, srec, int(f[4]), int(f[5])) == want, cmd
    # the arena: without SSIM tables the layout is the older one to the byte; with them two more regions, nothing overlapping
    shapes = [(3, 2), (0, 0), (64, 8), (257, 5), (1, 1), (0, 7)]
    flat = " ".join("%d %d" % s for s in shapes)
    n = len(shapes)
    for host in (0, 1):
        old, new = (([int(x) for x in line.split()]) for line in S.run_target2_host(exe, d, ["L %d 0 0 %s" % (host, flat), "L %d 32 64 %s" % (host, flat)]))
        assert old[4] == old[5] == old[6 + 0] and old[:4] + old[6:] == [int(x) for x in T.run_target_host(T.build_target_host(d), d, ["L %d %s" % (host, flat)])[0].split()]
        total, moves, jobs, records, sj, sr = new[:6]
        ranges = [(moves, 24 * 3 * n), (jobs, 32 * n), (records, 64 * n), (sj, 32 * n), (sr, 64 * n)]
        for i, (w, h) in enumerate(shapes):
            orig, best, bestf, img, filt = new[6 + 5 * i: 11 + 5 * i]
            rows = h if w else 0
            ranges += [(orig, w * h * 4), (best, w * h * 4), (bestf, rows)] + ([(img, w * h * 4), (filt, rows)] if host else [])
        assert all(a % 256 == 0 for a, _ in ranges)
        live = sorted((a, a + b) for a, b in ranges if b)
        assert all(x[1] <= y[0] for x, y in zip(live, live[1:])) and live[-1][1] <= total


def test_bad_targets_are_refused_without_a_device():
    lib = P.hip_lib()
    for s in (math.nan, -0.5, 1.5):
        t = P.Target2(35.0, 0, 19, s)
        assert lib.pngloss_hip_optimize_batch_target2(None, None, 0, C.byref(t), 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_multi_optimize_batch_host_target2(None, None, 0, C.byref(t), 2, None, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_optimize_batch_target2(None, None, 0, None, 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT


def test_new_entry_points_are_exported_and_declared():
    header = open(os.path.join(U.ROOT, "include", "pngloss_hip.h")).read()
    lib = C.CDLL(os.path.join(U.ROOT, "pngloss_amd", "csrc", "libpngloss_hip.so"))
    for name in ("pngloss_hip_last_ssim", "pngloss_hip_multi_last_ssim", "pngloss_hip_compare_batch_ssim", "pngloss_hip_optimize_batch_target2",
                 "pngloss_hip_multi_optimize_batch_host_target2"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in L.ABI_SYMBOLS, name
    assert re.search(r"\bdouble\s+pngloss_hip_ssim_mean\s*\(", header) and hasattr(lib, "pngloss_hip_ssim_mean")
    for name in ("pngloss_hip_ssim", "pngloss_hip_target2"):
        assert re.search(r"\}\s*%s\s*;" % name, header), name
    assert C.sizeof(P.Target2) == 24 and C.sizeof(P.Target) == 16


def _tool():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    return exe


@needs_cli
def test_help_names_both_switches():
    r = subprocess.run([_tool(), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--ssim" in r.stdout and "--target-ssim" in r.stdout


@needs_cli
def test_bad_target_ssim_values_are_refused_like_a_bad_strength(tmp_path):
    exe = _tool()
    bad_s = subprocess.run([exe, "-s", "abc", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    range_s = subprocess.run([exe, "-s", "300", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert bad_s.returncode == range_s.returncode == L.PNGLOSS_INVALID_ARGUMENT
    for args, like in ((["--target-ssim", "x"], bad_s), (["--target-ssim", ""], bad_s), (["--target-ssim", "0"], range_s), (["--target-ssim", "1.5"], range_s),
                       (["--target-ssim", "-0.5"], range_s), (["--target-ssim", "nan"], range_s), (["--target-psnr", "35", "--target-ssim", "0"], range_s)):
        r = subprocess.run([exe] + args + ["x.png"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == like.returncode, (args, r.stderr)
        assert r.stderr.strip() and len(r.stderr.splitlines()) == len(like.stderr.splitlines()) == 1, (args, r.stderr)      # one line of message, no file touched
    assert not os.listdir(tmp_path)

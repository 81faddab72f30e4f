"""CPU tests of the distortion report (no GPU compute): pngloss_hip_psnr_db on hand-made records, the kernel's arithmetic
(pngloss_amd/csrc/pl_distort_core.h) run on the CPU under the sanitizers against numpy, the launch shape (pld_grid_blocks) against its restatement, and the command line switch where no device is needed.
Expected values come from numpy / Python arithmetic (tests/util_distort.py), never from the code under test."""
import math
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists("/opt/conda/include/png.h") or os.path.exists("/usr/include/png.h")
needs_cli = pytest.mark.skipif(not have_png, reason="libpng headers not found on this box: the command line tool is not built")


def _rec(pixels, changed, sq, mx=(0, 0, 0, 0)):
    return dict(pixels=pixels, changed_pixels=changed, sq_err=list(sq), max_abs=list(mx))


def test_psnr_known_value_and_every_mask():
    # 100 pixels, every red sample off by 5: MSE over R alone is 25 -> 10 log10(65025 / 25) = 34.1514...
    r = _rec(100, 100, (2500, 0, 0, 0), (5, 0, 0, 0))
    assert P.psnr_db(r, 0x1) == pytest.approx(10.0 * math.log10(65025.0 / 25.0), rel=1e-12)
    assert P.psnr_db(r, 0x1) == pytest.approx(34.151403521958, rel=1e-12)
    # over all four channels the same error is spread over four times the samples: + 10 log10(4)
    assert P.psnr_db(r, 0xF) == pytest.approx(10.0 * math.log10(65025.0 * 4.0 / 25.0), rel=1e-12)
    rng = np.random.default_rng(5)
    for _ in range(50):
        px = int(rng.integers(1, 1 << 40))
        rec = _rec(px, px, [int(rng.integers(0, 65025)) * int(rng.integers(0, px + 1)) for _ in range(4)])
        for mask in range(1, 16):
            want, got = D.py_psnr_db(rec, mask), P.psnr_db(rec, mask)
            assert (math.isinf(want) and got == math.inf) or got == pytest.approx(want, rel=1e-12), (rec, mask)
    # the masks of the four byte-per-pixel classes
    assert P.PSNR_MASK_OF_BPP == {1: 0x2, 2: 0xA, 3: 0x7, 4: 0xF}
    d = P.Distortion(100, 100, (P.lib.C.c_uint64 * 4)(2500, 0, 0, 0), (P.lib.C.c_uint32 * 4)(5, 0, 0, 0))
    assert d.psnr_db(0x1) == P.psnr_db(r, 0x1) and d.as_dict() == r


def test_psnr_infinite_for_no_error_and_nan_for_no_answer():
    same = _rec(64, 0, (0, 0, 0, 0))
    for mask in range(1, 16):
        assert P.psnr_db(same, mask) == math.inf
    only_alpha = _rec(64, 3, (0, 0, 0, 12), (0, 0, 0, 2))
    assert P.psnr_db(only_alpha, 0x7) == math.inf and math.isfinite(P.psnr_db(only_alpha, 0x8))      # the error is outside the mask
    assert math.isnan(P.psnr_db(_rec(0, 0, (0, 0, 0, 0)), 0xF))
    assert math.isnan(P.psnr_db(same, 0)) and math.isnan(P.psnr_db(same, 0x10)) and math.isnan(P.psnr_db(same, 0xFFFFFFFF))
    assert math.isnan(P.hip_lib().pngloss_hip_psnr_db(None, 0xF))


def test_core_arithmetic_equals_numpy_under_asan_and_ubsan(tmp_path):
    """the kernel's thread loop on the CPU: the mixed shapes, misaligned bases, the sums beyond 2^32 and a lane that must flush its 32-bit sums"""
    exe = D.build_distort_host(tmp_path)
    rng = np.random.default_rng(3)
    cases = []
    for a, b in D.mixed_pairs():
        for nt in (1, 64, 8 * 256):
            cases.append((a, b, 0, 0, nt))
    a, b = D.mixed_pairs()[4]                                   # 257 x 5 from bases 4 bytes behind a 16-byte boundary: d_a, d_b, both
    assert a.shape == (5, 257, 4)
    cases += [(a, b, 4, 0, 256), (a, b, 0, 4, 256), (a, b, 4, 4, 256), (a, b, 12, 8, 7)]
    zeros, ones = np.zeros((2048, 2048, 4), np.uint8), np.full((2048, 2048, 4), 255, np.uint8)
    cases.append((zeros, ones, 0, 0, 2048 * 256))               # every sum 2048 * 2048 * 255^2 > 2^32
    last = zeros.copy()
    last[-1, -1, 3] = 1
    cases.append((zeros, last, 0, 0, 2048 * 256))
    cases.append((zeros[:160], ones[:160], 0, 0, 1))            # ONE lane takes 327 680 pixels of full error: five times what 32 bits hold
    cases.append((zeros[:160], ones[:160], 4, 0, 1))            # ... and through the word-by-word loop
    same = rng.integers(0, 256, (33, 65, 4), dtype=np.uint8)
    cases.append((same, same.copy(), 0, 0, 64))
    got = D.run_distort_host(exe, tmp_path, cases)
    for (a, b, oa, ob, nt), g in zip(cases, got):
        assert g == D.np_distortion(a, b), (a.shape, oa, ob, nt)
    assert got[len(D.MIXED_SHAPES) * 3 + 4]["sq_err"] == [2048 * 2048 * 255 * 255] * 4 == [272734617600] * 4


def test_grid_rule_equals_its_restatement_at_the_pinned_points(tmp_path):
    """pld_grid_blocks, PLD_MAX_IMAGES and PLD_THREADS of pl_distort_core.h -- what pl_distort.hip launches pl_keep and pl_distort with -- against
    D.grid_blocks, whose values at the pinned points are written out in D.GRID_POINTS"""
    exe = D.build_distort_host(tmp_path)
    assert D.GRID_N == [1, 5, 59, 255, 256, 257, 300, 65535] and sorted(D.GRID_POINTS) == [0, 1, 4096, 4097, 33587200]
    points = [(n, m) for m in sorted(D.GRID_POINTS) for n in D.GRID_N]
    points += [(n, m) for n in (2, 7, 8, 228, 229, 260, 2048, 2049, 65540) for m in (4095, 8192, 8193, 32768, 32769, 527857, 4096 * 2048, 4096 * 2048 + 1, 1 << 40)]
    max_images, threads, got = D.run_distort_grid(exe, points)
    assert (max_images, threads) == (D.MAX_IMAGES, D.THREADS) == (65535, 256)
    assert got == [D.grid_blocks(n, m) for n, m in points]
    assert got[: 5 * 8] == [b for m in sorted(D.GRID_POINTS) for b in D.GRID_POINTS[m]]
    # what the GPU tests rely on: in a batch of 256 or more an image has 2048 lanes, and 8192 x 4100 pixels are then 4100 quads a lane -- 16 pixels past
    # the first flush; alone it has 2048 workgroups and a lane never flushes
    assert D.lane_pixels(260, 8192 * 4100, 8192 * 4100) == 16400 == D.FLUSH_PIXELS + 16 and D.lane_pixels(260, 8192 * 4100, 8192 * 4100, vector=False) == 16400
    assert D.lane_pixels(1, 8192 * 4100, 8192 * 4100) == 68 < D.FLUSH_PIXELS      # 524 288 lanes, 17 quads at the most


@needs_cli
def test_help_names_the_switch():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--distortion" in r.stdout


@needs_cli
def test_switch_does_not_change_exit_codes(tmp_path):
    """argument errors, a missing file and a real file: the same exit code with and without --distortion -- on a box without a GPU the real file
    fails with the library's error either way, and the switch adds nothing to stderr there"""
    from PIL import Image
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    src = tmp_path / "a.png"
    Image.fromarray(P.synth_rgba(24, 10, 0, 1), "RGBA").save(src)
    no_gpu = P.hip_lib().pngloss_hip_device_count() <= 0
    for args in ([], ["-s", "300", "x.png"], ["-b", "0", "x.png"], ["--bogus"], ["-f", str(tmp_path / "missing.png")], ["-f", str(src)], ["-f", "--gpu-read", "--gpu-deflate", str(src)]):
        plain = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path, timeout=300)
        flag = subprocess.run([exe, "--distortion"] + args, capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert flag.returncode == plain.returncode, (args, plain.stderr[-300:], flag.stderr[-300:])
        if no_gpu and args:
            assert flag.stderr == plain.stderr, args
    if no_gpu:
        assert subprocess.run([exe, "--distortion", "-f", str(src)], capture_output=True, cwd=tmp_path).returncode == 64

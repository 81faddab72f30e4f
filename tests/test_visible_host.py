"""CPU tests of the visible measuring mode (no GPU compute): pm for every (c, A); the visible instantiation of the kernels' thread loops
(pngloss_amd/csrc/pl_distort_core.h, pl_ssim_core.h) run on the CPU under the sanitizers against numpy; visible records under the host helpers and
the acceptance rule; the evidence the mode rests on (dice at strength 19); the floors of the GPU search test; and the command line switch where no
device is needed.  Expected values come from numpy / Python arithmetic (tests/util_visible.py), never from the code under test; every comparison
of records is exact."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_distort as D
from tests import util_ssim as S
from tests import util_target as T
from tests import util_visible as V

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists("/opt/conda/include/png.h") or os.path.exists("/usr/include/png.h")
needs_cli = pytest.mark.skipif(not have_png, reason="libpng headers not found on this box: the command line tool is not built")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("visible_host")
    return V.build_visible_host(d), d


def test_pm_for_every_channel_value_and_alpha(harness):
    """numpy's pm and the C code's against exact rounding: the nearest integer to c * A / 255, never a tie, at most 255, alpha kept"""
    exe, _ = harness
    want = np.zeros((256, 256), np.int64)
    for alpha in range(256):
        for c in range(256):
            x = Fraction(c * alpha, 255)
            assert x - math.floor(x) != Fraction(1, 2)
            want[alpha, c] = math.floor(x + Fraction(1, 2))
    assert want.max() == 255 and (want[255] == np.arange(256)).all() and not want[0].any()
    px = np.zeros((256, 256, 4), np.uint8)
    px[..., 0] = px[..., 1] = px[..., 2] = np.arange(256)[None, :]
    px[..., 3] = np.arange(256)[:, None]
    got = V.pm(px)
    for c in range(3):
        assert np.array_equal(got[..., c], want)
    assert np.array_equal(got[..., 3], px[..., 3])
    words = want | want << 8 | want << 16 | np.arange(256, dtype=np.int64)[:, None] << 24
    assert np.array_equal(V.run_pm(exe).astype(np.int64), words)


def test_closed_forms_of_the_two_uniform_pairs_equal_the_visible_definition():
    """V.trip_expected() takes the SSIM records of the 66 048- and 66 049-window pairs from their 8x8 corner: the definition on the whole pairs agrees"""
    want = dict(zip([n for n, _, _ in V.trip_pairs()], V.trip_expected()))
    for name, a, b in V.trip_pairs():
        if name in ("1036x1028_checkerboard_inverse", "1032x1032_equal"):
            assert V.py_ssim(a, b) == want[name][1], name
            assert abs(want[name][1]["sum_q16"][0]) > 1 << 32 and want[name][1]["windows"] == S.geometry(a.shape[1], a.shape[0])[0] * S.geometry(a.shape[1], a.shape[0])[1]
    assert want["300x77_invisible"] == (dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4), V.NO_WINDOWS)


def test_distortion_loop_equals_numpy_under_asan_and_ubsan(harness):
    """the visible thread loop on the CPU: the mixed shapes, misaligned bases, a lane that must flush its 32-bit sums, nothing visible, pixels visible
    in one image only, and an opaque pair, whose visible record is the all-pixel one"""
    exe, d = harness
    cases = []
    for a, b in V.distort_pairs():
        for nt in (1, 64, 8 * 256):
            cases.append(("distort", a, b, 0, 0, nt))
    a, b = V.distort_pairs()[4]
    assert a.shape == (5, 257, 4)
    cases += [("distort", a, b, 4, 0, 256), ("distort", a, b, 0, 12, 256), ("distort", a, b, 4, 4, 256), ("distort", a, b, 12, 8, 7)]
    zeros, ones = np.zeros((160, 2048, 4), np.uint8), np.full((160, 2048, 4), 255, np.uint8)
    flush = len(cases)
    cases.append(("distort", zeros, ones, 0, 0, 1))             # ONE lane takes 327 680 visible pixels of full error: five times what 32 bits hold
    cases.append(("distort", zeros, ones, 4, 0, 1))             # ... and through the word-by-word loop
    edge = V.edge_pairs()
    first_edge = len(cases)
    for name in ("invisible", "alpha_0_3", "opaque"):
        cases.append(("distort", *edge[name], 0, 0, 64))
    got = V.run_visible_host(exe, d, cases)
    for (_, a, b, oa, ob, nt), g in zip(cases, got):
        assert g == V.np_distortion(a, b), (a.shape, oa, ob, nt)
    assert got[flush] == got[flush + 1] == dict(pixels=327680, changed_pixels=327680, sq_err=[327680 * 255 * 255] * 4, max_abs=[255] * 4)
    assert 327680 > 66051 * 4
    # nothing visible: nothing to measure, whatever the colours are
    assert got[first_edge] == dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)
    assert D.np_distortion(*edge["invisible"])["changed_pixels"] > 0
    # alpha 0 -> 3 and 3 -> 0: visible though one of the two images does not show them; the alpha error is 3 on every one of them
    a, b = edge["alpha_0_3"]
    assert got[first_edge + 1]["pixels"] == 8 * 24 + 8 * 12 == got[first_edge + 1]["changed_pixels"] and got[first_edge + 1]["sq_err"][3] == 9 * (8 * 24 + 8 * 12)
    assert got[first_edge + 1]["max_abs"][3] == 3 and max(got[first_edge + 1]["max_abs"][:3]) <= 3
    assert got[first_edge + 2] == D.np_distortion(*edge["opaque"])
    # a pair with transparency really differs from its all-pixel record
    a, b = V.distort_pairs()[5]
    assert V.np_distortion(a, b) != D.np_distortion(a, b) and 0 < V.np_distortion(a, b)["pixels"] < a.shape[0] * a.shape[1]


def test_ssim_loops_equal_python_integers_under_asan_and_ubsan(harness):
    """the two visible thread loops on the CPU: one window, none, a dropped window, a tile filled to the brim, two tiles each way on the word-by-word and on the 16-byte path,
    misaligned bases, nothing visible, an opaque pair"""
    exe, d = harness
    pairs = V.ssim_pairs()
    cases, names = [], []
    for name, (a, b) in pairs.items():
        for nt in (4, 64, 256):
            cases.append(("ssim", a, b, 0, 0, nt)); names.append(name)
    for name in ("133x37", "136x40", "137x41"):
        for oa, ob in ((4, 0), (12, 12)):
            cases.append(("ssim", *pairs[name], oa, ob, 256)); names.append(name)
    edge = V.edge_pairs()
    for name in ("invisible", "alpha_0_3", "opaque"):
        cases.append(("ssim", *edge[name], 0, 0, 256)); names.append(name)
    want = {name: V.py_ssim(a, b) for name, (a, b) in list(pairs.items()) + list(edge.items())}
    got = V.run_visible_host(exe, d, cases)
    for name, (_, a, b, oa, ob, nt), g in zip(names, cases, got):
        assert g == want[name], (name, oa, ob, nt)
    assert want["8x8"]["windows"] == 1 and want["7x64"] == V.NO_WINDOWS == want["invisible"]
    # 16 x 8: windows at x = 0, 4, 8; the first lies in the invisible columns -- and its q is not what the other two sum to
    a, b = pairs["16x8_left_invisible"]
    assert S.py_ssim(a, b)["windows"] == 3 and want["16x8_left_invisible"]["windows"] == 2
    # one tile filled to its last window origin; two tiles each way on either load path; windows without a visible pixel among them
    assert S.geometry(133, 37) == (32, 8) and S.geometry(136, 40) == S.geometry(137, 41) == (33, 9)
    for name, (w, h) in (("133x37", (133, 37)), ("136x40", (136, 40)), ("137x41", (137, 41))):
        nx, ny = S.geometry(w, h)
        assert 0 < want[name]["windows"] < nx * ny, name
    assert want["opaque"] == S.py_ssim(*edge["opaque"]) and want["opaque"]["windows"] == 9 * 5


def test_visible_records_under_the_host_helpers_and_the_acceptance_rule(tmp_path):
    """pngloss_hip_psnr_db, pngloss_hip_ssim_mean and pl_target_accept2 take visible records as they are; pixels == 0 is "nothing to measure" """
    nothing = dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)
    a, b = V.edge_pairs()["alpha_0_3"]
    recs = [nothing, V.np_distortion(a, b), V.np_distortion(*V.distort_pairs()[5]), V.np_distortion(*V.ssim_pairs()["136x40"]),
            dict(pixels=157, changed_pixels=100, sq_err=[2500, 0, 0, 0], max_abs=[5, 0, 0, 0])]
    srecs = [V.NO_WINDOWS, V.py_ssim(a, b), V.NO_WINDOWS, V.py_ssim(*V.ssim_pairs()["136x40"]), dict(windows=7, sum_q16=[7 * 65536 - 700] * 4, min_q16=[65000] * 4, reserved=0)]
    for mask in range(1, 16):
        assert math.isnan(P.psnr_db(nothing, mask)) and math.isnan(P.ssim_mean(V.NO_WINDOWS, mask))
        for rec in recs[1:]:
            want, got = D.py_psnr_db(rec, mask), P.psnr_db(rec, mask)
            assert (math.isinf(want) and got == math.inf) or got == pytest.approx(want, rel=1e-12), (rec, mask)
        for srec in (srecs[1], srecs[3], srecs[4]):
            assert P.ssim_mean(srec, mask) == pytest.approx(S.py_mean(srec, mask), rel=1e-12)
    # 157 visible pixels, every red sample of 100 of them off by 5: the mean is over the visible pixels, not over the 320 of the image
    assert P.psnr_db(recs[4], 0x1) == pytest.approx(10.0 * math.log10(65025.0 * 157 / 2500.0), rel=1e-12)
    # the acceptance rule itself (tests/c/target2_host.cpp runs pl_target_accept2) against the restatement the search replay uses
    exe = S.build_target2_host(tmp_path)
    commands, wants = [], []
    for rec, srec in zip(recs, srecs):
        for psnr, mx, ssim in ((0.0, 0, 0.0), (30.0, 0, 0.0), (60.0, 0, 0.0), (0.0, 2, 0.0), (0.0, 0, 0.97), (0.0, 0, 1.0), (20.0, 200, 0.5)):
            for bpp in (2, 4):
                commands.append("A %s %d %s 0 %d %d %s %s %d %s" % (T.double_bits(psnr), mx, T.double_bits(ssim), bpp, rec["pixels"], " ".join(map(str, rec["sq_err"])),
                                                                   " ".join(map(str, rec["max_abs"])), srec["windows"], " ".join(map(str, srec["sum_q16"]))))
                wants.append("1" if S.py_accept2(psnr, mx, ssim, rec, srec, 0, bpp) else "0")
    assert S.run_target2_host(exe, tmp_path, commands) == wants
    assert "0" in wants and "1" in wants
    assert all(w == "1" for w in wants[:14])            # nothing visible: every target is met


def test_dice_is_worse_where_it_shows_than_the_all_pixel_psnr_says():
    """the evidence behind the mode: the suite's dice image through the CPU oracle at strength 19"""
    img = U.load_npz("suite_inputs.npz")["dice"]
    assert 0.3 < (img[..., 3] != 0).mean() < 0.35
    out, _ = U.run_port(img, 19, 2)
    rec, vrec = D.np_distortion(img, out), V.np_distortion(img, out)
    assert vrec["pixels"] < rec["pixels"]
    assert D.py_psnr_db(vrec, 0xF) < D.py_psnr_db(rec, 0xF)


def test_floors_of_the_search_test_separate_the_two_modes():
    """what tests/test_gpu_visible.py searches for: on the CPU oracle at least one image ends at another strength under "visible" than under "all",
    and both conditions decide somewhere"""
    all_px = [V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, V.SEARCH_SSIM, False)[0] for i in range(3)]
    vis = [V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, V.SEARCH_SSIM, True)[0] for i in range(3)]
    assert any(a != v for a, v in zip(all_px, vis)), (all_px, vis)
    assert all(0 < v < V.SEARCH_M for v in vis)
    assert vis != [V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, 0.0, True)[0] for i in range(3)]
    assert vis != [V.oracle_search(i, V.SEARCH_M, 0.0, V.SEARCH_SSIM, True)[0] for i in range(3)]
    for i, img in enumerate(V.batch_images()):
        share = (img[..., 3] != 0).mean()
        assert 0.2 < share < 0.8 and img.shape[:2] == V.BATCH_SHAPES[i][::-1]


def test_library_exports_the_entry_point_and_the_header_declares_it():
    assert "pngloss_hip_compare_batch_visible" in L.ABI_SYMBOLS
    assert P.hip_lib().pngloss_hip_compare_batch_visible is not None
    with open(os.path.join(U.ROOT, "include", "pngloss_hip.h")) as fh:
        header = fh.read()
    assert "int pngloss_hip_compare_batch_visible(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out_distortion," in header
    assert hasattr(P.HipContext, "compare_visible")


def _tool():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    return exe


@needs_cli
def test_help_names_the_switch():
    r = subprocess.run([_tool(), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--visible" in r.stdout


@needs_cli
def test_visible_without_anything_to_measure_is_an_argument_error(tmp_path):
    """like the refused --target-size combinations: the tool's exit code for bad arguments, one line on stderr, no file touched"""
    exe = _tool()
    for args in (["--visible"], ["--visible", "-s", "19", "-f"], ["--visible", "--gpu-deflate"], ["--visible", "--target-size", "4k"],
                 ["--visible", "--distortion", "--target-size", "4k"]):
        r = subprocess.run([exe] + args + ["x.png"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == L.PNGLOSS_INVALID_ARGUMENT, (args, r.returncode, r.stderr)
        assert "--visible" in r.stderr and len(r.stderr.splitlines()) == 1, (args, r.stderr)
    # with something to measure the switch gets past the argument checks: the file does not exist (a read error, not an argument error)
    for extra in (["--distortion"], ["--ssim"], ["--target-psnr", "35"], ["--max-error", "8"], ["--target-ssim", "0.9"]):
        r = subprocess.run([exe, "--visible"] + extra + ["missing.png"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode not in (0, L.PNGLOSS_INVALID_ARGUMENT) and "cannot open" in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.listdir(tmp_path)

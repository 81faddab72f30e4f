"""GPU tests of the quantiser's premultiplied space (include/pngloss_hip_quant_space.h): the four *3 calls against the restatement of
tests/util_quant_space.py -- pixels, entries, palette, exact, colors_in and the visible-mode record, by equality --, over the CPU cases and the device
shapes at which a workgroup takes a second chunk, one bin holds every colour, the search loop's unroll ends; space 0 through the new calls against
the older calls; dithering over a band boundary; the colour-count search with its visible records, an image with nothing to see among them; the
refusal of a space that is none; and the tool's --colors-visible."""
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_quant as Q
from tests import util_quant_space as S
from tests import util_visible as V

pytestmark = pytest.mark.gpu

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
FS = P.lib.DITHER_FLOYD_STEINBERG
VISIBLE = P.lib.QUANT_SPACE_VISIBLE


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def multi():
    m = P.HipMulti("0,0")
    yield m
    m.close()


def _upload(arrays):
    import torch
    dev = []
    for a in arrays:
        buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        view = buf[:a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        dev.append((buf, view))
    torch.cuda.synchronize()
    return dev, [(v.data_ptr() if a.size else 0, 0, a.shape[1], a.shape[0]) for (_, v), a in zip(dev, arrays)]


def _download(dev, arrays):
    import torch
    torch.cuda.synchronize()
    for (buf, _), a in zip(dev, arrays):
        assert not buf[a.size:].any().item()                        # nothing is written behind an image
    return [v.cpu().numpy().reshape(a.shape) for (_, v), a in zip(dev, arrays)]


def _run(ctx, arrays, n, rounds=8, dither=None, space=VISIBLE):
    dev, descs = _upload(arrays)
    _, reports = ctx.quantize(descs, n, rounds, dither=dither, space=space)
    return _download(dev, arrays), reports


def _target_run(ctx, arrays, m, psnr=0.0, max_abs=0, rounds=8, dither=0, space=VISIBLE):
    dev, descs = _upload(arrays)
    _, reports = ctx.quantize_target(descs, P.lib.QuantTarget(psnr, max_abs), m, rounds, dither, space=space)
    return _download(dev, arrays), reports


def _alpha_randomised(img, seed):
    """the image with its alpha byte drawn anew: a third of the pixels invisible, a third opaque, a third anything"""
    rng = np.random.default_rng(seed)
    out = img.copy()
    pick = rng.random(img.shape[:2])
    out[..., 3] = np.where(pick < 1 / 3, 0, np.where(pick < 2 / 3, 255, rng.integers(0, 256, img.shape[:2]))).astype(np.uint8)
    return out


def _shapes():
    """name -> (image, max_colors, rounds)"""
    out = {"crop_4": (S.crop(), 4, 8), "crop_16": (S.crop(), 16, 8), "dirty_8": (S.dirty(), 8, 8)}
    out.update(S.small_shapes())
    device = Q.device_shapes()
    for name in ["one_bin_299_colours", "rose_3", "rose_5", "rose_7"] + list(_last_pixel_names()):
        out[name] = device[name]
    img, n, rounds = device["3x1100_300_colours"]
    out["3x1100_300_colours_alpha"] = (_alpha_randomised(img, 71), n, rounds)
    return out


def _last_pixel_names():
    from tests.util_index import last_pixel_images
    return last_pixel_images().keys()


SHAPES = {}


def _shape(name):
    if not SHAPES:
        SHAPES.update(_shapes())
    return SHAPES[name]


SHAPE_NAMES = ["crop_4", "crop_16", "dirty_8", "1x1", "1x7", "5x1", "transparent_row_r0", "transparent_row_r8", "low_alpha", "one_bin_299_colours", "rose_3", "rose_5",
               "rose_7", "3x1100_300_colours_alpha", "last_pixel_images"]


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_device_and_host_forms_against_the_restatement(ctx, multi, name):
    names = list(_last_pixel_names()) if name == "last_pixel_images" else [name]
    for k in names:
        img, n, rounds = _shape(k)
        want = S.restate(img, n, rounds)
        outs, reports = _run(ctx, [img], n, rounds)
        assert np.array_equal(outs[0], want["pixels"]), k
        S.same_report(k, reports[0], want)
        host_outs, host_reports = multi.quantize_host([img], n, rounds, space=VISIBLE)
        assert np.array_equal(host_outs[0], want["pixels"]) and host_reports[0] == reports[0], k


def test_a_workgroup_takes_a_second_chunk_in_a_batch(ctx):
    batch, n, rounds = Q.device_shapes()["two_chunks_in_a_batch"]
    assert len(batch) == 256 and Q.busiest_wg_pixels(100 * 100, 256) >= 2 * Q.CHUNK
    outs, reports = _run(ctx, batch, n, rounds)
    for i, (img, out, rep) in enumerate(zip(batch, outs, reports)):
        want = S.restate(img, n, rounds)
        assert np.array_equal(out, want["pixels"]), i
        S.same_report(i, rep, want)


def _nothing_to_see():
    rng = np.random.default_rng(67)
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., :3] = rng.permutation(64).reshape(8, 8, 1) * 3
    return img


def test_a_batch_of_exact_invisible_and_working_images(ctx, multi):
    flat = Q.shapes()["flat_64x16"][0]
    arrays = [flat, _nothing_to_see(), S.crop(), np.zeros((0, 0, 4), np.uint8), S.dirty()]
    outs, reports = _run(ctx, arrays, 16, 8)
    host_outs, host_reports = multi.quantize_host(arrays, 16, 8, space=VISIBLE)
    for i, (img, out, rep) in enumerate(zip(arrays, outs, reports)):
        want = S.restate(img, 16, 8)
        assert np.array_equal(out, want["pixels"]) and np.array_equal(host_outs[i], out) and host_reports[i] == rep, i
        S.same_report(i, rep, want)
    assert [r["exact"] for r in reports] == [1, 0, 0, 1, 0]
    assert not outs[1].any() and reports[1]["entries"] == 1 and reports[1]["palette"] == [0] and reports[1]["distortion"]["pixels"] == 0
    assert reports[0]["distortion"]["pixels"] == 64 * 16 and reports[0]["distortion"]["changed_pixels"] == 0


def test_space_0_through_the_new_calls_is_the_older_call(ctx, multi):
    arrays = [S.crop(), S.tall(), Q.shapes()["flat_64x16"][0]]
    for dither in (0, FS):
        old_outs, old_reports = _run(ctx, arrays, 5, 2, dither=dither, space=None)
        new_outs, new_reports = _run(ctx, arrays, 5, 2, dither=dither, space=P.lib.QUANT_SPACE_RGBA)
        host_outs, host_reports = multi.quantize_host(arrays, 5, 2, dither=dither, space=P.lib.QUANT_SPACE_RGBA)
        for i in range(len(arrays)):
            assert np.array_equal(old_outs[i], new_outs[i]) and old_reports[i] == new_reports[i] == host_reports[i] and np.array_equal(old_outs[i], host_outs[i]), (dither, i)
        assert not np.array_equal(new_outs[0], _run(ctx, arrays[:1], 5, 2, dither=dither)[0][0])     # ... and space 1 is another image
    old = _target_run(ctx, arrays[:1], 64, 33.0, space=None)
    new = _target_run(ctx, arrays[:1], 64, 33.0, space=P.lib.QUANT_SPACE_RGBA)
    assert np.array_equal(old[0][0], new[0][0]) and old[1] == new[1]
    host = multi.quantize_host_target(arrays[:1], P.lib.QuantTarget(33.0), 64, 8, space=P.lib.QUANT_SPACE_RGBA)
    assert np.array_equal(old[0][0], host[0][0]) and old[1] == host[1]


@pytest.mark.parametrize("name,n,rounds", [("crop", 4, 8), ("crop", 16, 8), ("tall", 5, 2)])
def test_dithered_against_the_restatement(ctx, multi, name, n, rounds):
    img = S.crop() if name == "crop" else S.tall()
    want = S.restate(img, n, rounds, 1)
    outs, reports = _run(ctx, [img], n, rounds, dither=FS)
    assert np.array_equal(outs[0], want["pixels"]), name
    S.same_report(name, reports[0], want)
    host_outs, host_reports = multi.quantize_host([img], n, rounds, dither=FS, space=VISIBLE)
    assert np.array_equal(host_outs[0], outs[0]) and host_reports[0] == reports[0]
    assert not np.array_equal(outs[0], S.restate(img, n, rounds)["pixels"])


PROBES = {}


def _probes(dither=0):
    if dither not in PROBES:
        PROBES[dither] = S.Probes(S.crop(), 8, dither)
    return PROBES[dither]


@pytest.mark.parametrize("psnr,max_abs,dither", [(33.0, 0, 0), (0.0, 40, 0), (30.0, 0, FS)])
def test_search_against_the_restated_procedure(ctx, multi, psnr, max_abs, dither):
    p = _probes(1 if dither else 0)
    want = p.search(64, psnr, max_abs)
    refused = [n for k, n in enumerate(want["probed"]) if not want["accepted_mask"] >> k & 1]
    print(want["colors"], want["probed"], bin(want["accepted_mask"]), [round(p.psnr(n), 3) for n in want["probed"]])
    assert want["probes"] >= 3 and refused and want["reached"] == 1
    assert not psnr or min(abs(p.psnr(n) - psnr) for n in want["probed"]) >= 1e-6          # C's and Python's log10 cannot disagree on a probe
    outs, reports = _target_run(ctx, [S.crop()], 64, psnr, max_abs, 8, dither)
    S.same_target_report((psnr, max_abs, dither), reports[0], want)
    assert np.array_equal(outs[0], want["quant"]["pixels"])
    plain_outs, plain_reports = _run(ctx, [S.crop()], reports[0]["colors"], 8, dither=dither)      # the call at the chosen N, on a fresh copy
    assert np.array_equal(outs[0], plain_outs[0]) and reports[0]["quant"] == plain_reports[0]
    host_outs, host_reports = multi.quantize_host_target([S.crop()], P.lib.QuantTarget(psnr, max_abs), 64, 8, dither, space=VISIBLE)
    assert np.array_equal(host_outs[0], outs[0]) and host_reports[0] == reports[0]


def test_search_on_an_image_with_nothing_to_see(ctx):
    img = _nothing_to_see()
    flat = Q.shapes()["flat_64x16"][0]
    want = S.Probes(img).search(16, 40.0)
    assert (want["colors"], want["reached"], want["probed"], want["accepted_mask"]) == (2, 1, [16, 8, 4, 2], 0xF)
    outs, reports = _target_run(ctx, [img, flat], 16, 40.0)
    S.same_target_report("nothing to see", reports[0], want)
    assert reports[0]["quant"]["distortion"]["pixels"] == 0 and not outs[0].any() and reports[0]["quant"]["exact"] == 0
    # an exact image beside it: every probe without device work, and the probe's `pixels` is the visible count of the result's record
    S.same_target_report("flat", reports[1], S.Probes(flat).search(16, 40.0))
    assert reports[1]["quant"]["exact"] == 1 and reports[1]["probe_distortion"]["pixels"] == reports[1]["quant"]["distortion"]["pixels"] == 64 * 16


def test_a_space_that_is_none_is_refused_on_a_live_context(ctx, multi):
    img = S.crop()
    dev, descs = _upload([img])
    for space in (2, 255, 0xFFFFFFFF):
        with pytest.raises(RuntimeError):
            ctx.quantize(descs, 16, 8, space=space)
        with pytest.raises(RuntimeError):
            ctx.quantize_target(descs, P.lib.QuantTarget(30.0), 16, 8, space=space)
        with pytest.raises(RuntimeError):
            multi.quantize_host([img], 16, 8, space=space)
        with pytest.raises(RuntimeError):
            multi.quantize_host_target([img], P.lib.QuantTarget(30.0), 16, 8, space=space)
    with pytest.raises(RuntimeError):
        ctx.quantize(descs, 16, 8, dither=2, space=VISIBLE)
    assert np.array_equal(_download(dev, [img])[0], img)


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")
def test_tool_quantises_in_the_premultiplied_space(tmp_path):
    from PIL import Image
    img = S.crop()
    want = S.restate(img, 16, 8)
    src, out = str(tmp_path / "crop.png"), str(tmp_path / "crop-16.png")
    Image.fromarray(img, "RGBA").save(src)
    assert np.array_equal(np.asarray(Image.open(src).convert("RGBA")), img)
    r = subprocess.run([OUR_CLI, "-f", "--colors", "16", "--colors-visible", "--distortion", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    pixels = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(pixels, want["pixels"])
    lines = r.stderr.splitlines()
    at = lines.index("  colors: more than 256 in the input, %d palette entries" % want["entries"])
    assert lines[at + 1] == "  colour space: premultiplied"
    assert V.cli_lines(want["distortion"], V.NO_WINDOWS, 4)[0] in lines, r.stderr
    # without the switch: the plain quantiser's file and the line over all pixels
    r = subprocess.run([OUR_CLI, "-f", "--colors", "16", "--distortion", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "colour space" not in r.stderr and "(visible)" not in r.stderr
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), Q.restate(img, 16, 8)["pixels"])
    r = subprocess.run([OUR_CLI, "-f", "--colors-visible", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == P.lib.PNGLOSS_INVALID_ARGUMENT and r.stderr == "--colors-visible requires --colors.\n"

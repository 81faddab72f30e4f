"""GPU tests of the colour quantiser (include/pngloss_hip_quant.h): pngloss_hip_quantize_batch and its multi host form against the restatement of
tests/util_quant.py -- pixels, palette, colors_in, entries, exact, and the distortion record against tests/util_distort.py, all by equality --, a
batch against its images run alone, then the way to a palette file: the option "indexed" behind the quantiser, and the tool's --colors."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D
from tests import util_index as X
from tests import util_quant as Q

pytestmark = pytest.mark.gpu

SHAPES = Q.shapes()
NAMES = list(SHAPES)
OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
BATCH_N, BATCH_R = 16, 8


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


def _device_run(ctx, images, n, rounds, offset_words=0):
    """quantise copies of `images` on the device; offset_words: the device pointers are that many words past a 16-byte boundary.  Returns
    (pixels, reports)"""
    import torch
    dev = []
    for a in images:
        buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        view = buf[4 * offset_words: 4 * offset_words + a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        dev.append((buf, view))
    torch.cuda.synchronize()
    descs = [(v.data_ptr() if a.size else 0, 0, a.shape[1], a.shape[0]) for (_, v), a in zip(dev, images)]
    _, reports = ctx.quantize(descs, n, rounds)
    torch.cuda.synchronize()
    outs = [v.cpu().numpy().reshape(a.shape) for (_, v), a in zip(dev, images)]
    for (buf, _), a in zip(dev, images):          # nothing is written outside the image
        assert not buf[:4 * offset_words].any().item() and not buf[4 * offset_words + a.size:].any().item()
    return outs, reports


def _same(name, img, got_pixels, got, want):
    assert np.array_equal(got_pixels, want["pixels"]), name
    assert got["status"] == 0, name
    assert (got["colors_in"], got["entries"], got["exact"]) == (want["colors_in"], want["entries"], want["exact"]), name
    assert got["palette"] == want["palette"], name
    assert got["distortion"] == want["distortion"] == D.np_distortion(img, want["pixels"]), name


@pytest.fixture(scope="module")
def want():
    """the restatement of every shape at its own parameters: computed once"""
    return {name: Q.restate(img, n, rounds) for name, (img, n, rounds) in SHAPES.items()}


@pytest.mark.parametrize("name", NAMES)
def test_shape_against_the_restatement(ctx, want, name):
    img, n, rounds = SHAPES[name]
    outs, reports = _device_run(ctx, [img], n, rounds)
    _same(name, img, outs[0], reports[0], want[name])
    if name == "3x3_two_colours_exact":
        assert reports[0]["exact"] == 1 and reports[0]["distortion"]["changed_pixels"] == 0 and np.array_equal(outs[0], img)
    if name == "noise_257x33":
        assert img.shape[1] % 4 and img.shape[0] * img.shape[1] > 1024 and reports[0]["exact"] == 0       # a ragged tail, more than one workgroup


def test_device_pointers_off_the_16_byte_boundary(ctx, want):
    for name in ("noise_257x33", "rose_16", "5x1"):
        img, n, rounds = SHAPES[name]
        for off in (1, 3):
            outs, reports = _device_run(ctx, [img], n, rounds, offset_words=off)
            _same(name, img, outs[0], reports[0], want[name])


def _batch_images():
    seen, images = set(), []
    for name, (img, _, _) in SHAPES.items():
        if id(img) not in seen:
            seen.add(id(img))
            images.append((name, img))
    images.insert(3, ("empty", np.zeros((0, 0, 4), np.uint8)))
    images.append(("empty_rows", np.zeros((0, 5, 4), np.uint8)))
    return images


@pytest.fixture(scope="module")
def batch(ctx):
    images = _batch_images()
    outs, reports = _device_run(ctx, [img for _, img in images], BATCH_N, BATCH_R)
    return images, outs, reports


def test_batch_equals_each_image_alone_and_the_restatement(ctx, batch):
    images, outs, reports = batch
    assert any(r["exact"] for r in reports) and not all(r["exact"] for r in reports)
    for (name, img), out, rep in zip(images, outs, reports):
        one_out, one_rep = _device_run(ctx, [img], BATCH_N, BATCH_R)
        assert np.array_equal(out, one_out[0]) and rep == one_rep[0], name
        w = Q.restate(img, BATCH_N, BATCH_R)
        assert np.array_equal(out, w["pixels"]), name
        assert (rep["colors_in"], rep["entries"], rep["exact"], rep["palette"], rep["distortion"]) == (w["colors_in"], w["entries"], w["exact"], w["palette"], w["distortion"]), name
        if not img.size:
            assert (rep["colors_in"], rep["entries"], rep["exact"], rep["palette"]) == (0, 0, 1, []) and rep["distortion"]["pixels"] == 0, name


def test_multi_host_form_equals_the_device_form(batch):
    """two contexts on device 0: the report of images[i] comes from whichever context image i went to, the pixels come back where they were"""
    images, outs, reports = batch
    arrays = [img for _, img in images]
    assert set(P.multi_split([(a.shape[1], a.shape[0]) for a in arrays], 2)) == {0, 1}
    m = P.HipMulti("0,0")
    try:
        host_outs, host_reports = m.quantize_host(arrays, BATCH_N, BATCH_R)
        with pytest.raises(RuntimeError):
            m.quantize_host(arrays, 1, 8)
        with pytest.raises(RuntimeError):
            m.quantize_host(arrays, 257, 8)
        with pytest.raises(RuntimeError):
            m.quantize_host(arrays, 16, 65)
    finally:
        m.close()
    for (name, _), a, b, ra, rb in zip(images, outs, host_outs, reports, host_reports):
        assert np.array_equal(a, b) and ra == rb, name


def test_refusals_on_a_live_context(ctx):
    img = SHAPES["rose_16"][0]
    for n, rounds in ((1, 8), (257, 8), (0, 8), (16, 65)):
        with pytest.raises(RuntimeError):
            _device_run(ctx, [img], n, rounds)
    with pytest.raises(RuntimeError):
        ctx.quantize([(0, 0, 4, 4)], 16, 8)            # pixels, and no pointer


# ---- end to end: a palette file ----

@pytest.mark.parametrize("name", ["rose_16", "rose_256", "noise_257x33"])
def test_quantised_image_goes_out_indexed(ctx, want, name):
    img, n, rounds = SHAPES[name]
    m = P.HipMulti("0")
    try:
        outs, reports = m.quantize_host([img], n, rounds)
    finally:
        m.close()
    _same(name, img, outs[0], reports[0], want[name])
    ctx.set_option("indexed", "on")
    try:
        pix, _, zs = ctx.run_host_zlib([outs[0]], 0, 2)
        pal = ctx.palette(0).as_dict()
    finally:
        ctx.set_option("indexed", "off")
    assert np.array_equal(pix[0], outs[0])                                  # strength 0 changes no pixel
    ctype, stream, _ = zs[0]
    assert ctype == 3 and pal["entries"] == reports[0]["entries"] <= n and pal["colors"] == reports[0]["entries"]
    restated = X.restate(outs[0])
    assert [int(x) for x in restated["words"]] == reports[0]["palette"] and pal["plte"] == restated["plte"] and pal["trns"] == restated["trns"]
    rows = zlib.decompress(stream)
    h, w = img.shape[:2]
    assert len(rows) == h * (w + 1) and rows == restated["scanlines"]
    idx = np.frombuffer(rows, np.uint8).reshape(h, w + 1)
    assert not idx[:, 0].any()
    assert np.array_equal(Q.from_words(np.array(reports[0]["palette"], np.uint32)[idx[:, 1:].reshape(-1)], w, h), outs[0])


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")
def test_tool_writes_a_palette_file_of_16_colours(tmp_path, want):
    from PIL import Image
    img = SHAPES["rose_16"][0]
    src, out = str(tmp_path / "rose.png"), str(tmp_path / "rose-16.png")
    Image.fromarray(img, "RGBA").save(src)
    r = subprocess.run([OUR_CLI, "-f", "--colors", "16", "--distortion", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    im = Image.open(out)
    assert im.mode == "P"
    pixels = np.asarray(im.convert("RGBA"))
    w = want["rose_16"]
    assert np.array_equal(pixels, w["pixels"]) and len(np.unique(Q.words(pixels))) == w["entries"] <= 16
    ch = dict(X.chunks_of(open(out, "rb").read()))
    assert ch[b"IHDR"][8:10] == b"\x08\x03" and len(ch[b"PLTE"]) == 3 * w["entries"]
    lines = r.stderr.splitlines()
    assert "  colors: more than 256 in the input, 16 palette entries" in lines
    assert D.cli_line(w["distortion"], 3) in lines, r.stderr                # (rose is opaque colour: three stored channels)
    # a second file that already has few colours comes back exact, and says so
    exact_src, exact_out = str(tmp_path / "flat.png"), str(tmp_path / "flat-16.png")
    Image.fromarray(SHAPES["3x3_two_colours_exact"][0], "RGBA").save(exact_src)
    r = subprocess.run([OUR_CLI, "-f", "--colors", "16", "--distortion", "-v", "-o", exact_out, exact_src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    assert "  colors: 2 in the input, 2 palette entries, exact (no pixel changed)" in r.stderr.splitlines() and "  distortion: none (lossless)" in r.stderr.splitlines()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(open(exact_out, "rb").read())).convert("RGBA")), SHAPES["3x3_two_colours_exact"][0])

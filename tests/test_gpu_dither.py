"""GPU tests of the quantiser's error diffusion (include/pngloss_hip_dither.h): pngloss_hip_quantize_batch2 and its multi host form with dither = 1
against the raster-order restatement of tests/util_dither.py -- pixels and the whole report, by equality --, on shapes that each cross one boundary
of the kernel's schedule, behind an assertion from the restated constants that they do; dither = 0 against the old calls; device pointers off the
16-byte boundary, a batch against its images alone, the caller's stream, the refusals, a regrown workspace; then the way to a palette file: the
option "indexed" behind the dithered image, and the tool's --colors N --dither."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D
from tests import util_dither as F
from tests import util_index as X
from tests import util_quant as Q

pytestmark = pytest.mark.gpu

SHAPES = F.shapes()
NAMES = list(SHAPES)
OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
BATCH_N, BATCH_R = 4, 2
FS = P.lib.DITHER_FLOYD_STEINBERG


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


def _device_run(ctx, images, n, rounds, dither=FS, offset_words=0):
    """quantise copies of `images` on the device; offset_words: the device pointers are that many words past a 16-byte boundary.  Returns
    (pixels, reports); nothing may be written outside an image"""
    import torch
    dev = []
    for a in images:
        buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        view = buf[4 * offset_words: 4 * offset_words + a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        dev.append((buf, view))
    torch.cuda.synchronize()
    descs = [(v.data_ptr() if a.size else 0, 0, a.shape[1], a.shape[0]) for (_, v), a in zip(dev, images)]
    _, reports = ctx.quantize(descs, n, rounds, dither=dither)
    torch.cuda.synchronize()
    outs = [v.cpu().numpy().reshape(a.shape) for (_, v), a in zip(dev, images)]
    for (buf, _), a in zip(dev, images):
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
    out = {}
    for name, (img, n, rounds) in SHAPES.items():
        stats = {}
        out[name] = F.restate(img, n, rounds, stats)
        out[name]["stats"] = stats
    return out


def _crosses(name, img, want):
    """the shape does cross the boundary it is there for, by the restated constants"""
    h, w = img.shape[:2]
    K, BAND, LANES = F.K, F.BAND, F.LANES
    if name == "1x3":
        assert (w, h) == (1, 3) and SHAPES[name][1] == 2
    elif name == "1x_band_plus_1":
        assert w == 1 and h == BAND + 1 and h > F.WAVES * LANES                    # row `band` belongs to a second band
    elif name == "2K_plus_1_x1":
        assert h == 1 and w == 2 * K + 1 and (w - 1) // K == 2                      # lane 0, whose column is its local step, walks into a third epoch
    elif name == "2x2":
        assert (w, h) == (2, 2)
    elif name.endswith("x65"):
        assert h == LANES + 1 and w in (K - 1, K, K + 1) and F.barriers(w, h) == F.wave_epochs(w) + F.LAG          # a second wave with rows
    elif name == "3x_two_bands_plus_1":
        assert w == 3 and h == 2 * BAND + 1 and -(-h // BAND) == 3 and w < 2 * LANES                              # lanes whose columns are all out of range
    elif name == "3K_plus_5":
        assert w == 3 * K + 5 and h == BAND + 2 and h > BAND and F.wave_epochs(w) > F.LAG
    elif name == "ring_wraps":
        assert w == F.RING + 5 and h == BAND + 2 and w > F.RING and h > BAND         # columns RING .. RING + 4 fall on the slots of columns 0 .. 4
    elif name.startswith("rose_"):
        n = SHAPES[name][1]
        assert len(F.final_palette(img, n, SHAPES[name][2])) == n and (n % 4 or n in (16, 256))
    elif name == "tux_16":
        # transparent pixels beside opaque ones.  (Its alpha is 0 or 255 and so is every entry's: on this image the alpha errors are all zero.  The
        # noise shapes have alpha in every value, and there it diffuses: the alpha plane differs from that of the nearest-entry image)
        assert len(np.unique(img[..., 3])) == 2 and len(np.unique(want["pixels"][..., 3])) == 2
        noise, n, rounds = SHAPES["65x65"]
        assert not np.array_equal(Q.restate(noise, n, rounds)["pixels"][..., 3], F.restate(noise, n, rounds)["pixels"][..., 3])
    elif name == "clamp":
        assert want["stats"]["a_min"] < 0 and want["stats"]["a_max"] > 255
    else:
        raise AssertionError(name)
    assert want["exact"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_shape_against_the_restatement(ctx, want, name):
    img, n, rounds = SHAPES[name]
    _crosses(name, img, want[name])
    outs, reports = _device_run(ctx, [img], n, rounds)
    _same(name, img, outs[0], reports[0], want[name])


def test_dithering_differs_from_the_nearest_entry_image(ctx, want):
    """(the tests above would pass on a kernel that diffused nothing only if the restatement did not either)"""
    img, n, rounds = SHAPES["rose_16"]
    plain = Q.restate(img, n, rounds)
    assert not np.array_equal(plain["pixels"], want["rose_16"]["pixels"]) and plain["entries"] <= want["rose_16"]["entries"] <= n


def test_device_pointers_off_the_16_byte_boundary(ctx, want):
    for name in ("65x65", "rose_16", "2K_plus_1_x1"):
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
    two = np.array([0xFF102030, 0xFFE0D0C0], np.uint32)
    images.insert(6, ("exact", Q.from_words(two[[0, 1, 1, 0, 0, 1, 1, 1, 0]], 3, 3)))
    return images


@pytest.fixture(scope="module")
def batch(ctx):
    images = _batch_images()
    outs, reports = _device_run(ctx, [img for _, img in images], BATCH_N, BATCH_R)
    return images, outs, reports


def test_batch_equals_each_image_alone_and_the_restatement(ctx, batch, want):
    images, outs, reports = batch
    assert len(images) == len(set(id(a) for _, a in images)) >= 14
    for (name, img), out, rep in zip(images, outs, reports):
        one_out, one_rep = _device_run(ctx, [img], BATCH_N, BATCH_R)
        assert np.array_equal(out, one_out[0]) and rep == one_rep[0], name
        own = name in SHAPES and SHAPES[name][1:] == (BATCH_N, BATCH_R)          # (the large shapes run at the batch's parameters: restated once)
        _same(name, img, out, rep, want[name] if own else F.restate(img, BATCH_N, BATCH_R))
        if not img.size:
            assert (rep["colors_in"], rep["entries"], rep["exact"], rep["palette"]) == (0, 0, 1, []) and rep["distortion"]["pixels"] == 0, name
        if name in ("exact", "1x3", "2x2"):                         # at most BATCH_N colours: never dithered
            assert rep["exact"] == 1 and np.array_equal(out, img) and rep["distortion"]["changed_pixels"] == 0, name
    assert sum(r["exact"] for r in reports) == 5 and not all(r["exact"] for r in reports)


def test_dither_0_through_the_new_calls_is_the_old_calls(ctx):
    shapes = Q.shapes()
    m = P.HipMulti("0")
    try:
        for name, (img, n, rounds) in shapes.items():
            old_out, old_rep = _device_run(ctx, [img], n, rounds, dither=None)
            new_out, new_rep = _device_run(ctx, [img], n, rounds, dither=P.lib.DITHER_NONE)
            assert np.array_equal(old_out[0], new_out[0]) and old_rep == new_rep, name
            host_old, host_old_rep = m.quantize_host([img], n, rounds)
            host_new, host_new_rep = m.quantize_host([img], n, rounds, dither=P.lib.DITHER_NONE)
            assert np.array_equal(host_old[0], host_new[0]) and host_old_rep == host_new_rep == old_rep and np.array_equal(host_old[0], old_out[0]), name
    finally:
        m.close()


def test_multi_host_form_equals_the_device_form(batch):
    """two contexts on device 0: the report of images[i] comes from whichever context image i went to, the pixels come back where they were"""
    images, outs, reports = batch
    arrays = [img for _, img in images]
    assert set(P.multi_split([(a.shape[1], a.shape[0]) for a in arrays], 2)) == {0, 1}
    m = P.HipMulti("0,0")
    try:
        host_outs, host_reports = m.quantize_host(arrays, BATCH_N, BATCH_R, dither=FS)
        for bad in ((1, 8, FS), (257, 8, FS), (16, 65, FS), (16, 8, 2)):
            with pytest.raises(RuntimeError):
                m.quantize_host(arrays, bad[0], bad[1], dither=bad[2])
    finally:
        m.close()
    for (name, _), a, b, ra, rb in zip(images, outs, host_outs, reports, host_reports):
        assert np.array_equal(a, b) and ra == rb, name


def test_refusals_on_a_live_context(ctx):
    import torch
    img = SHAPES["rose_16"][0]
    for n, rounds, dither in ((1, 8, FS), (257, 8, FS), (16, 65, FS), (16, 8, 2), (16, 8, 0xFFFFFFFF)):
        with pytest.raises(RuntimeError):
            _device_run(ctx, [img], n, rounds, dither=dither)
    with pytest.raises(RuntimeError):
        ctx.quantize([(0, 0, 4, 4)], 16, 8, dither=FS)            # pixels, and no pointer
    d = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    rep = (P.lib.QuantReport * 1)()
    descs = (P.lib.ImageDesc * 1)(P.lib.ImageDesc(d.data_ptr(), None, img.shape[1], img.shape[0]))
    params = P.lib.QuantParams2(16, 8, FS, 1)                       # reserved not 0
    assert P.hip_lib().pngloss_hip_quantize_batch2(ctx._ctx, descs, 1, C.byref(params), rep, None) == P.lib.PNGLOSS_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(img.shape), img)


def test_a_batch_in_flight_is_refused_and_nothing_is_written(want):
    import torch
    frame = P.synth_rgba(160, 48, 0, 1)
    port_out, port_filters = U.run_port(frame, 19, 2)
    name = "rose_16"
    img, n, rounds = SHAPES[name]
    ctx = P.HipContext()
    try:
        d = torch.from_numpy(frame.reshape(-1).copy()).cuda()
        f = torch.zeros(48, dtype=torch.uint8, device="cuda")
        other = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        desc = [(other.data_ptr(), 0, img.shape[1], img.shape[0])]
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), 160, 48)], 19, 2)
        with pytest.raises(RuntimeError):
            ctx.quantize(desc, n, rounds, dither=FS)
        res = ctx.finish()
        torch.cuda.synchronize()
        assert np.array_equal(other.cpu().numpy().reshape(img.shape), img)                   # the refused call wrote nothing
        assert res[0]["status"] == 0 and np.array_equal(d.cpu().numpy().reshape(frame.shape), port_out) and np.array_equal(f.cpu().numpy(), port_filters)
        _, reports = ctx.quantize(desc, n, rounds, dither=FS)                                  # ... and left the context usable
        torch.cuda.synchronize()
        _same(name, img, other.cpu().numpy().reshape(img.shape), reports[0], want[name])
    finally:
        ctx.close()


def test_a_regrown_workspace_keeps_nothing_of_the_call_before(want):
    """one context: a wide image of two bands, then a small one, then the wide one again -- no palette, ring or error line of a call shows in the next"""
    wide, small = "ring_wraps", "2x2"
    ctx = P.HipContext()
    try:
        runs = [_device_run(ctx, [SHAPES[k][0]], SHAPES[k][1], SHAPES[k][2]) for k in (wide, small, wide, small)]
    finally:
        ctx.close()
    for k, (outs, reports) in zip((wide, small, wide, small), runs):
        _same(k, SHAPES[k][0], outs[0], reports[0], want[k])


def test_the_work_goes_to_the_callers_stream(ctx, want):
    """the image reaches its buffer only through work enqueued on the caller's stream, right in front of the call and with no synchronisation in
    between: a call that put its kernels on another stream would find the zeros the buffer held before -- an exact, flat image.  Correct code
    passes whatever the timing: everything is ordered by the one stream"""
    import torch
    name = "65x65"
    img, n, rounds = SHAPES[name]
    staged = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
    buf = torch.zeros(img.size, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for k in range(256):                        # some 16 GiB of stores in front of the copy: milliseconds of work in flight
            scratch.fill_(k % 251)
        buf.copy_(staged, non_blocking=True)
        _, reports = ctx.quantize([(buf.data_ptr(), 0, img.shape[1], img.shape[0])], n, rounds, stream=st.cuda_stream, dither=FS)
    st.synchronize()
    torch.cuda.synchronize()
    assert int(scratch[-1].item()) == 255 % 251
    _same(name, img, buf.cpu().numpy().reshape(img.shape), reports[0], want[name])
    assert reports[0]["exact"] == 0                                                           # (zeros would have come back exact)


# ---- end to end: a palette file ----

def test_dithered_image_goes_out_indexed(ctx, want):
    name = "rose_16"
    img, n, rounds = SHAPES[name]
    m = P.HipMulti("0")
    try:
        outs, reports = m.quantize_host([img], n, rounds, dither=FS)
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
    assert ctype == 3 and pal["entries"] == reports[0]["entries"] <= n
    rows = zlib.decompress(stream)
    h, w = img.shape[:2]
    assert len(rows) == h * (w + 1)
    idx = np.frombuffer(rows, np.uint8).reshape(h, w + 1)
    assert not idx[:, 0].any()
    assert np.array_equal(Q.from_words(np.array(reports[0]["palette"], np.uint32)[idx[:, 1:].reshape(-1)], w, h), outs[0])


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")
def test_tool_writes_a_dithered_palette_file(tmp_path):
    from PIL import Image
    img = SHAPES["rose_16"][0]
    w = F.restate(img, 16, 8)                                               # (the tool's rounds: PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS)
    src, out = str(tmp_path / "rose.png"), str(tmp_path / "rose-16.png")
    Image.fromarray(img, "RGBA").save(src)
    r = subprocess.run([OUR_CLI, "-f", "--colors", "16", "--dither", "--distortion", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    im = Image.open(out)
    assert im.mode == "P"
    pixels = np.asarray(im.convert("RGBA"))
    assert np.array_equal(pixels, w["pixels"]) and len(np.unique(Q.words(pixels))) == w["entries"] <= 16
    ch = dict(X.chunks_of(open(out, "rb").read()))
    assert ch[b"IHDR"][8:10] == b"\x08\x03" and len(ch[b"PLTE"]) == 3 * w["entries"]
    lines = r.stderr.splitlines()
    at = lines.index("  colors: more than 256 in the input, %d palette entries" % w["entries"])
    assert lines[at + 1] == "  dither: Floyd-Steinberg"
    assert D.cli_line(w["distortion"], 3) in lines, r.stderr                # (rose is opaque colour: three stored channels)
    r = subprocess.run([OUR_CLI, "-f", "--dither", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == P.lib.PNGLOSS_INVALID_ARGUMENT and r.stderr == "--dither requires --colors.\n"

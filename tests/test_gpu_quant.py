"""GPU tests of the colour quantiser (include/pngloss_hip_quant.h): pngloss_hip_quantize_batch and its multi host form against the restatement of
tests/util_quant.py -- pixels, palette, colors_in, entries, exact, and the distortion record against tests/util_distort.py, all by equality --, a
batch against its images run alone; the shapes of Q.device_shapes(), at which a workgroup takes more than one chunk, a channel sum passes 2^32, the cut
ends with one entry and the deciding colour lies in one pixel -- each behind an assertion, from the restated grid rule, that the shape does so --;
the caller's stream, a batch in flight and a regrown workspace; then the way to a palette file: the option "indexed" behind the quantiser, and the
tool's --colors."""
import ctypes as C
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


# ---- the loops past one trip, the sums past 32 bits (Q.device_shapes) ----

@pytest.fixture(scope="module")
def device():
    return Q.device_shapes()


@pytest.fixture(scope="module")
def device_want(device):
    """name -> the restatement of a device shape (a list for a batch), computed when a test first asks and then shared"""
    class Cache(dict):
        def __missing__(self, name):
            img, n, rounds = device[name]
            self[name] = [Q.restate(a, n, rounds) for a in img] if isinstance(img, list) else Q.restate(img, n, rounds)
            return self[name]
    return Cache()


def _pixels(img):
    return img.shape[0] * img.shape[1]


def test_a_workgroup_takes_a_second_chunk_of_a_single_image(ctx, device, device_want):
    """2113 chunks: a single image would like 2048 workgroups and gets the 1024 a launch has at most, so every workgroup of pl_quant_hist,
    pl_quant_assign and pl_quant_remap goes round its loop twice, 65 of them three times, and keeps its cells across the chunks"""
    name = "two_chunks_single"
    img, n, rounds = device[name]
    chunks, nblocks = -(-_pixels(img) // Q.CHUNK), Q.blocks(_pixels(img), Q.want_blocks(1))
    assert Q.want_blocks(1) == 2048 and chunks == 2113 and nblocks == min(2048, Q.MAX_BLOCKS) == 1024 and chunks - 2 * nblocks == 65
    assert Q.busiest_wg_pixels(_pixels(img), 1) == 3 * Q.CHUNK >= 2 * Q.CHUNK
    assert device_want[name]["exact"] == 0 and device_want[name]["entries"] > 128
    for off in (0, 1):
        outs, reports = _device_run(ctx, [img], n, rounds, offset_words=off)
        _same(f"{name} at offset {off}", img, outs[0], reports[0], device_want[name])


@pytest.fixture(scope="module")
def small_and_large_batch(ctx, device):
    images, n, rounds = device["two_chunks_in_a_batch"]
    return _device_run(ctx, images, n, rounds)


def test_a_workgroup_takes_a_second_chunk_in_a_batch(ctx, device, device_want, small_and_large_batch):
    """256 working images get 8 workgroups each, and the grid is sized by the one large image in the middle: two of its workgroups take two of its
    10 chunks, every workgroup of a small image but the first leaves at once"""
    name = "two_chunks_in_a_batch"
    images, n, rounds = device[name]
    large = [i for i, a in enumerate(images) if _pixels(a) > 4]
    assert len(images) == 256 and large == [127] and _pixels(images[127]) == 100 * 100
    assert all(w["exact"] == 0 for w in device_want[name])                                    # every image is a working image
    assert Q.want_blocks(256) == 8 and Q.blocks(100 * 100, 8) == 8 and -(-100 * 100 // Q.CHUNK) == 10
    assert Q.busiest_wg_pixels(100 * 100, 256) >= 2 * Q.CHUNK
    outs, reports = small_and_large_batch
    for i, (img, out, rep, w) in enumerate(zip(images, outs, reports, device_want[name])):
        _same(f"{name}[{i}]", img, out, rep, w)
        one_out, one_rep = _device_run(ctx, [img], n, rounds)
        assert np.array_equal(out, one_out[0]) and rep == one_rep[0], i


def test_channel_sums_past_32_bits(ctx, device, device_want):
    """one entry takes every bright pixel of 18.9 million: its accumulators are past 2^32, which only the 64-bit flush and the 64-bit update
    carry.  The image also holds 0x00000000 and 0xFFFFFFFF: |c|^2 = 0 and p.c = 4 * 255^2, the ends of the key arithmetic"""
    name = "sums_past_32_bits"
    img, n, rounds = device[name]
    w, want = Q.words(img), device_want[name]
    assert [int(x) for x in np.unique(w)] == [0x00000000, 0xFFFEFDFC, 0xFFFFFFFF] and (n, rounds) == (2, 2)
    bright = w[w != 0]
    sums = [int(((bright >> (8 * c)) & 255).astype(np.int64).sum()) for c in range(4)]
    print(name, "channel sums of the bright pixels", sums)
    assert sums[0] > 1 << 32 and min(sums) > 1 << 32
    assert want["entries"] == 2 and want["palette"][0] == 0 and want["palette"][1] >> 24 == 0xFF and want["exact"] == 0
    assert Q.busiest_wg_pixels(_pixels(img), 1) >= 2 * Q.CHUNK and 255 * Q.busiest_wg_pixels(_pixels(img), 1) < 1 << 32
    outs, reports = _device_run(ctx, [img], n, rounds)
    _same(name, img, outs[0], reports[0], want)


def test_more_colours_than_entries_in_one_histogram_bin(ctx, device, device_want):
    """299 colours of one bin: the cut cannot split its only box and ends with ONE entry, whatever N is"""
    for name in ("one_bin_299_colours", "one_bin_299_colours_to_2"):
        img, n, rounds = device[name]
        assert len(np.unique(Q.words(img))) >= 257 and len(Q.median_cut(Q.histogram(Q.words(img)), n)) == 1
        outs, reports = _device_run(ctx, [img], n, rounds)
        _same(name, img, outs[0], reports[0], device_want[name])
        assert (reports[0]["entries"], reports[0]["exact"], reports[0]["colors_in"]) == (1, 0, 257) and len(np.unique(Q.words(outs[0]))) == 1
    assert device_want["one_bin_299_colours"]["palette"] == device_want["one_bin_299_colours_to_2"]["palette"]
    assert np.array_equal(device_want["one_bin_299_colours"]["pixels"], device_want["one_bin_299_colours_to_2"]["pixels"])


@pytest.mark.parametrize("n", [3, 5, 7, 255])
def test_entry_counts_around_the_unroll_of_the_search(ctx, device, device_want, n):
    name = f"rose_{n}"
    img, max_colors, rounds = device[name]
    first = Q.median_cut(Q.histogram(Q.words(img)), max_colors)
    assert max_colors == n and len(first) == n and n % 4                                      # the search runs over n entries: no multiple of four
    outs, reports = _device_run(ctx, [img], max_colors, rounds)
    _same(name, img, outs[0], reports[0], device_want[name])


@pytest.mark.parametrize("name", ["257th_in_the_last_pixel", "257th_in_the_first_pixel", "256th_in_the_last_pixel"])
def test_the_deciding_colour_in_one_pixel(ctx, device, device_want, name):
    """59 chunks over the 32 workgroups of pl_index_count, which re-read the counter before each chunk and each insertion: the colour that
    decides between exact and not lies in the last pixel of the last chunk, or in the first of the first"""
    img, n, rounds = device[name]
    assert n == 256 and -(-_pixels(img) // Q.CHUNK) == 59
    outs, reports = _device_run(ctx, [img], n, rounds)
    _same(name, img, outs[0], reports[0], device_want[name])
    if name.startswith("257th"):
        assert len(np.unique(Q.words(img))) == 257
        assert (reports[0]["colors_in"], reports[0]["exact"]) == (257, 0) and reports[0]["entries"] <= 256 and len(np.unique(Q.words(outs[0]))) <= 256
    else:
        assert len(np.unique(Q.words(img))) == 256 and int((Q.words(img) == Q.words(img)[-1]).sum()) == 1
        assert (reports[0]["colors_in"], reports[0]["exact"], reports[0]["entries"]) == (256, 1, 256) and np.array_equal(outs[0], img)
        assert len(reports[0]["palette"]) == 256


# ---- the caller's stream, a batch in flight, the workspace ----

def test_the_work_goes_to_the_callers_stream(ctx, want):
    """the image reaches its buffer only through work enqueued on the caller's stream, right in front of the call and with no synchronisation in
    between: a call that put its kernels on another stream would find the zeros the buffer held before -- an exact, flat image.  Correct
    code passes whatever the timing: everything is ordered by the one stream"""
    import torch
    name = "noise_257x33"
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
        _, reports = ctx.quantize([(buf.data_ptr(), 0, img.shape[1], img.shape[0])], n, rounds, stream=st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    assert int(scratch[-1].item()) == 255 % 251
    _same(name, img, buf.cpu().numpy().reshape(img.shape), reports[0], want[name])
    assert reports[0]["exact"] == 0 and len(np.unique(Q.words(img))) > n                     # (zeros would have come back exact)


def test_quantize_refuses_a_batch_in_flight_and_touches_nothing(want):
    import torch
    frame = P.synth_rgba(160, 48, 0, 1)
    port_out, port_filters = U.run_port(frame, 19, 2)
    name = "rose_16"
    img, n, rounds = SHAPES[name]
    lib = P.hip_lib()
    ctx = P.HipContext()
    try:
        d = torch.from_numpy(frame.reshape(-1).copy()).cuda()
        f = torch.zeros(48, dtype=torch.uint8, device="cuda")
        other = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        desc = [(other.data_ptr(), 0, img.shape[1], img.shape[0])]
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), 160, 48)], 19, 2)
        rep = (P.lib.QuantReport * 1)()
        params = P.lib.QuantParams(n, rounds)
        descs = (P.lib.ImageDesc * 1)(P.lib.ImageDesc(other.data_ptr(), None, img.shape[1], img.shape[0]))
        assert lib.pngloss_hip_quantize_batch(ctx._ctx, descs, 1, C.byref(params), rep, None) == P.lib.PNGLOSS_INVALID_ARGUMENT
        with pytest.raises(RuntimeError):
            ctx.quantize(desc, n, rounds)
        res = ctx.finish()
        torch.cuda.synchronize()
        assert np.array_equal(other.cpu().numpy().reshape(img.shape), img)                   # the refused call wrote nothing
        assert res[0]["status"] == 0 and np.array_equal(d.cpu().numpy().reshape(frame.shape), port_out) and np.array_equal(f.cpu().numpy(), port_filters)
        _, reports = ctx.quantize(desc, n, rounds)                                            # ... and left the context usable
        torch.cuda.synchronize()
        _same(name, img, other.cpu().numpy().reshape(img.shape), reports[0], want[name])
    finally:
        ctx.close()


def test_a_regrown_workspace_keeps_nothing_of_the_call_before(device, device_want, want):
    """one context: 256 images, then one of five pixels, then 2.2 million pixels, then the five again -- no table, histogram, palette or accumulator
    of a larger call shows in a smaller one behind it"""
    batch, bn, br = device["two_chunks_in_a_batch"]
    big, gn, gr = device["two_chunks_single"]
    small, sn, sr = SHAPES["5x1"]
    ctx = P.HipContext()
    try:
        outs, reports = _device_run(ctx, batch, bn, br)
        first = _device_run(ctx, [small], sn, sr)
        big_outs, big_reports = _device_run(ctx, [big], gn, gr)
        second = _device_run(ctx, [small], sn, sr)
    finally:
        ctx.close()
    assert np.array_equal(first[0][0], second[0][0]) and first[1] == second[1]
    _same("5x1", small, first[0][0], first[1][0], want["5x1"])
    _same("two_chunks_single", big, big_outs[0], big_reports[0], device_want["two_chunks_single"])
    for i, (img, out, rep, w) in enumerate(zip(batch, outs, reports, device_want["two_chunks_in_a_batch"])):
        _same(f"batch[{i}]", img, out, rep, w)


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

@pytest.mark.parametrize("name", ["rose_16", "rose_256", "noise_257x33", "two_chunks_single", "3x1100_300_colours"])
def test_quantised_image_goes_out_indexed(ctx, want, device, device_want, name):
    """(the last two: a second chunk in the quantiser and then a second trip over the rows, or over a row, of pl_index_rows)"""
    img, n, rounds = SHAPES[name] if name in SHAPES else device[name]
    restated = want[name] if name in SHAPES else device_want[name]
    if name == "two_chunks_single":
        assert n == 256 and img.shape[0] > X.ROW_BLOCKS and img.shape[1] > X.ROW_PASS
    if name == "3x1100_300_colours":
        assert n == 5 and img.shape[:2] == (1100, 3) and len(np.unique(Q.words(img))) > 256
    m = P.HipMulti("0")
    try:
        outs, reports = m.quantize_host([img], n, rounds)
    finally:
        m.close()
    _same(name, img, outs[0], reports[0], restated)
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

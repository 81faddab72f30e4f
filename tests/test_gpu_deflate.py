"""GPU deflate (pngloss_hip_optimize_batch_host_zlib) through the C ABI: the zlib stream of every image must inflate
to exactly the scanlines the _emit call returns (i.e. to what libpng would have been handed by the reference,
rwpng.c:477-637), must be byte-identical to the CPU run of the same encoder core (tests/c/deflate_host.cpp), and must
not be larger than zlib level 9 / Z_FILTERED on image-sized inputs.
The second half feeds the device pipeline (dfl_pack, the radix sort with its flag / max-scan stage, dfl_match over the sorted order of a whole group of
images, dfl_encode with its 256-thread team, dfl_gather, dfl_sizes) the byte streams on which deflate goes wrong -- matches at the window's edge and
across a block boundary, streams around one block, symbol counts that need the code-length limit, identical neighbours, images shorter than a key --
carried by one-row opaque gray images at strength 0, and a seeded campaign over eight kinds of content."""
import functools
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext(0)
    yield c
    c.close()


def stream_of(emitted):
    ctype, ids, rows = emitted
    return np.concatenate([ids[:, None], rows], axis=1).tobytes() if rows.size else b""


def run_both(ctx, arrays, s=19, b=2, want_filters=True):
    outs, filts, emitted = ctx.run_host_emit(arrays, s, b, want_filters)
    outs2, filts2, streams = ctx.run_host_zlib(arrays, s, b, want_filters)
    for a, c in zip(outs, outs2):
        assert np.array_equal(a, c)
    return emitted, streams


def test_streams_inflate_to_the_emitted_scanlines_all_modes(ctx):
    arrays = [P.synth_rgba(96, 64, m, f) for m in range(6) for f in range(2)]
    emitted, streams = run_both(ctx, arrays)
    for e, (ctype, z, blocks) in zip(emitted, streams):
        assert ctype == e[0]
        assert zlib.decompress(z) == stream_of(e)
        assert sum(blocks) == 1


def test_streams_are_byte_identical_to_the_cpu_run_of_the_core(ctx):
    arrays = [P.synth_rgba(w, h, m, 3) for (w, h, m) in [(200, 150, 0), (333, 211, 1), (640, 480, 2), (257, 129, 3), (512, 300, 4), (301, 77, 5)]]
    emitted, streams = run_both(ctx, arrays)
    for e, (ctype, z, blocks) in zip(emitted, streams):
        want, stats = U.deflate_host(stream_of(e))
        assert z == want
        assert tuple(int(x) for x in stats[:3]) == blocks


def test_edge_shapes_and_empty_images(ctx):
    shapes = [(1, 1), (2, 3), (5, 1), (1, 7), (700, 1), (1, 700), (3, 3)]
    arrays = [P.synth_rgba(w, h, 0, 2) for (w, h) in shapes] + [np.zeros((0, 5, 4), np.uint8), np.zeros((4, 0, 4), np.uint8)]
    emitted, streams = run_both(ctx, arrays)
    for i, (e, (ctype, z, blocks)) in enumerate(zip(emitted, streams)):
        if arrays[i].size == 0:
            assert z == b""
            continue
        assert zlib.decompress(z) == stream_of(e)
        assert z == U.deflate_host(stream_of(e))[0]


def test_multi_block_images_adaptive_mode_and_strengths(ctx):
    # 1080p RGBA: 8.3 MB of scanlines = 32 deflate blocks; also all-rows-adaptive mode and other strengths
    big = P.synth_rgba(1920, 1080, 0, 0)
    emitted, streams = run_both(ctx, [big])
    data = stream_of(emitted[0])
    ctype, z, blocks = streams[0]
    assert zlib.decompress(z) == data and sum(blocks) == -(-len(data) // 262144)
    assert len(z) <= 0.95 * len(U.zlib9_filtered(data))            # measured: 6.1 % smaller than zlib level 9
    small = [P.synth_rgba(320, 200, 0, 1)]
    for s, b, wf in [(0, 2, True), (40, 2, True), (255, 1, True), (19, 2, False)]:
        emitted, streams = run_both(ctx, small, s, b, wf)
        assert zlib.decompress(streams[0][1]) == stream_of(emitted[0])


def test_incompressible_and_constant_content(ctx):
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (300, 400, 4), dtype=np.uint8)
    flat = np.full((300, 400, 4), 200, np.uint8)
    emitted, streams = run_both(ctx, [noise, flat], 0, 2)           # strength 0: pixels unchanged
    for e, (ctype, z, blocks) in zip(emitted, streams):
        assert zlib.decompress(z) == stream_of(e)
    assert streams[0][2][0] >= 1                                    # noise: stored blocks
    assert len(streams[0][1]) <= len(stream_of(emitted[0])) + 64
    assert len(streams[1][1]) < 2000


def test_mixed_batch_matches_single_image_calls(ctx):
    arrays = [P.synth_rgba(w, h, m, 7) for (w, h, m) in [(64, 64, 0), (1000, 600, 0), (17, 900, 2), (800, 31, 4), (256, 256, 1)]]
    _, batch = run_both(ctx, arrays)
    for a, got in zip(arrays, batch):
        _, single = run_both(ctx, [a])
        assert single[0] == got


def test_batches_split_into_several_groups(tmp_path):
    """A call handles at most 1 GiB of scanlines at a time and walks through larger batches in groups; a small group
    size (test hook PNGLOSS_HIP_DEFLATE_GROUP_BYTES) makes that path run with a handful of images."""
    import os
    import subprocess
    import sys
    code = (
        "import sys, zlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import pngloss_amd as P\n"
        "from tests import util as U\n"
        "ctx = P.HipContext(0)\n"
        "arrays = [P.synth_rgba(w, h, m, 9) for (w, h, m) in [(300, 200, 0), (64, 64, 1), (500, 400, 2), (31, 17, 3), (400, 300, 5), (200, 100, 0), (128, 128, 4)]]\n"
        "outs, filts, emitted = ctx.run_host_emit(arrays)\n"
        "outs2, filts2, streams = ctx.run_host_zlib(arrays)\n"
        "for e, (ctype, z, blocks) in zip(emitted, streams):\n"
        "    data = np.concatenate([e[1][:, None], e[2]], axis=1).tobytes()\n"
        "    assert ctype == e[0] and zlib.decompress(z) == data and z == U.deflate_host(data)[0]\n"
        "print('groups ok')\n" % U.ROOT)
    env = dict(os.environ, PNGLOSS_HIP_DEFLATE_GROUP_BYTES="300000", PNGLOSS_HIP_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "groups ok" in r.stdout, r.stderr[-800:]
    assert r.stderr.count("pngloss_hip deflate:") >= 4          # the seven images went through several groups


def test_stream_only_leaves_the_host_pixels_alone(ctx):
    a = P.synth_rgba(300, 200, 0, 4)
    outs, filts, streams = ctx.run_host_zlib([a], stream_only=True)
    assert np.array_equal(outs[0], a) and not filts[0].any()           # nothing was copied back ...
    _, _, full = ctx.run_host_zlib([a])
    assert streams[0] == full[0]                                       # ... and the stream is the same


def test_too_small_a_buffer_is_refused(ctx):
    """capacity < what the stream needs: PNGLOSS_INVALID_ARGUMENT (4), nothing written past the buffer"""
    import ctypes as C
    from pngloss_amd import lib as L
    a = np.ascontiguousarray(np.random.default_rng(8).integers(0, 256, (64, 64, 4), dtype=np.uint8))
    filt = np.zeros(64, np.uint8)
    buf = np.full(512, 0xAB, np.uint8)                      # a 64x64 noise image needs ~16 KB
    imgs = (L.HostImage * 1)(L.HostImage(a.ctypes.data, filt.ctypes.data, 64, 64))
    zs = (L.ZStream * 1)(L.ZStream(buf.ctypes.data, 256, 0, -1, (C.c_uint32 * 3)(0, 0, 0), 0))
    res = (L.Result * 1)()
    rc = ctx._lib.pngloss_hip_optimize_batch_host_zlib(ctx._ctx, imgs, 1, 0, 2, res, zs)
    assert rc == 4 and zs[0].size == 0
    assert (buf[256:] == 0xAB).all()
    assert ctx._lib.pngloss_hip_zlib_bound(64, 64) >= 64 * (64 * 4 + 1) + 11


# ---- hostile byte streams ------------------------------------------------------------------------------------------
# The carrier: an opaque gray image (R = G = B = v, A = 255) of height 1 at strength 0.  Its pixels stay as they are, it is written as colour type 0,
# one byte per pixel behind one filter byte, and only "none" or "sub" can be chosen for its row (libpng drops the others in a one-row image): both keep
# the periods and runs of v.

def carrier(values):
    v = np.frombuffer(bytes(values), np.uint8) if not isinstance(values, np.ndarray) else values.astype(np.uint8)
    assert 0 < v.size < (1 << 20)
    return np.ascontiguousarray(np.stack([v, v, v, np.full_like(v, 255)], axis=1)[None])


@functools.lru_cache(maxsize=None)
def tiled_chunk(period, total, seed=41):
    chunk = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8)
    return carrier(np.tile(chunk, total // period + 1)[:total])


@functools.lru_cache(maxsize=None)
def block_size_image(kind, width):
    return carrier(np.full(width, 77, np.uint8) if kind == "constant" else np.random.default_rng(42).integers(0, 256, width, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def fibonacci_values():
    """the 28 Fibonacci symbol counts of tests/test_deflate_host.py::test_code_length_limit (832039 bytes), the largest count on the value of the smallest
    magnitude (0, 1, 255, 2, 254, ...), so that "none" has the smaller sum, shuffled"""
    fib = [1, 1]
    while len(fib) < 28:
        fib.append(fib[-1] + fib[-2])
    by_magnitude = [0] + [v for k in range(1, 15) for v in (k, 256 - k)][:27]
    syms = np.concatenate([np.full(c, v, np.uint8) for c, v in zip(sorted(fib, reverse=True), by_magnitude)])
    np.random.default_rng(3).shuffle(syms)
    return syms


_cpu_cache = {}


def cpu_core(img):
    """(stream, z, block kinds) of a strength-0 image from the restatement and the CPU run of the encoder core; computed once per image"""
    key = id(img)
    if key not in _cpu_cache:
        assert img.shape[0] == 1                                       # (row 0 is adaptive in both row_filters modes)
        ctype, ids, rows = U.png_scanlines_reference(img, None)
        assert ctype == 0 and ids[0] in (0, 1)
        stream = stream_of((ctype, ids, rows))
        z, stats = U.deflate_host(stream)
        _cpu_cache[key] = (img, stream, z, tuple(int(x) for x in stats[:3]), int(stats[3]))
    return _cpu_cache[key][1:4]


def cpu_tokens(img):
    cpu_core(img)
    return _cpu_cache[id(img)][4]


def measure_only(ctx, imgs, want_filters):
    """pngloss_hip_optimize_batch_size as "strength 0, stream wanted": max_strength 0 and a budget no stream meets.  Per image (bytes, stream record)."""
    import torch
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    flt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") if want_filters else None for a in imgs]
    desc = [(d.data_ptr(), f.data_ptr() if f is not None else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)]
    res, rep, streams = ctx.run_size(desc, [1] * len(imgs), 0, 2, want_streams=True)
    torch.cuda.synchronize()
    for a, d, r in zip(imgs, dev, rep):
        assert (r.strength, r.probes, r.reached) == (0, 1, 0) and np.array_equal(d.cpu().numpy(), a)
    return [(int(r.bytes), st) for r, st in zip(rep, streams)]


def check_carriers(ctx, imgs):
    """every check of a hostile stream, in both row_filters modes; returns per image what cpu_core gives"""
    want = [cpu_core(a) for a in imgs]
    for want_filters in (True, False):
        outs, filts, emitted = ctx.run_host_emit(imgs, 0, 2, want_filters)
        outs2, _, streams = ctx.run_host_zlib(imgs, 0, 2, want_filters)
        measured = measure_only(ctx, imgs, want_filters)
        for i, a in enumerate(imgs):
            stream, z_cpu, kinds = want[i]
            ctype, z, blocks = streams[i]
            assert np.array_equal(outs[i], a) and np.array_equal(outs2[i], a), (i, want_filters)          # pixels unchanged
            assert ctype == 0 and emitted[i][0] == 0, (i, want_filters)
            assert stream_of(emitted[i]) == stream, (i, want_filters)                                      # scanlines == restatement
            assert zlib.decompress(z) == stream, (i, want_filters)
            assert z == z_cpu and blocks == kinds, (i, want_filters, len(z), len(z_cpu), blocks, kinds)
            assert measured[i][0] == len(z) and measured[i][1] == (0, z, blocks), (i, want_filters, measured[i][0], len(z))
    return want


@pytest.mark.parametrize("period", [32768, 32767, 32768 - 257, 32768 - 258, 32769])
def test_matches_at_the_far_edge_of_the_window(ctx, period):
    """a random chunk twice and 300 bytes more: every match is `period` back.  32768 is the farthest deflate can say, 32768 - 258 lets a longest match end
    at the window's edge, 32769 is out of reach.  (zlib level 9 finds none of these: it keeps 262 bytes of the window back.)"""
    img = tiled_chunk(period, 2 * period + 300)
    stream, z, kinds = cpu_core(img)
    print("far matches, period %d: block kinds %s, %d -> %d bytes, ratio %.4f" % (period, kinds, len(stream), len(z), len(z) / len(stream)))
    if period <= 32768:
        assert kinds == (0, 0, 1) and len(z) < 0.55 * len(stream)
    else:
        assert kinds == (1, 0, 0)
    check_carriers(ctx, [img])


def test_far_matches_across_a_block_boundary(ctx):
    """a 32768-byte chunk over 262144 + 5000 bytes: the matches of the second block's first 32 KiB point into the first block"""
    img = tiled_chunk(32768, 262144 + 5000)
    stream, z, kinds = cpu_core(img)
    print("far matches across blocks: block kinds %s, %d -> %d bytes, ratio %.4f" % (kinds, len(stream), len(z), len(z) / len(stream)))
    assert kinds == (0, 0, 2) and len(z) < 40000
    check_carriers(ctx, [img])


#: (kind, width) -> (stored, fixed, dynamic) blocks of the CPU core.  The stream is one filter byte longer than the width: 262143, 262144 (one whole
#: block), 262145 (a last block of a single byte) and 524288 (two whole blocks).
BLOCK_KINDS = {("constant", 262142): (0, 0, 1), ("constant", 262143): (0, 0, 1), ("constant", 262144): (0, 1, 1), ("constant", 524287): (0, 0, 2),
               ("noise", 262142): (1, 0, 0), ("noise", 262143): (1, 0, 0), ("noise", 262144): (1, 1, 0), ("noise", 524287): (2, 0, 0)}


@pytest.mark.parametrize("kind,width", sorted(BLOCK_KINDS), ids=["%s_%d" % k for k in sorted(BLOCK_KINDS)])
def test_streams_of_exactly_one_and_two_blocks_and_a_byte_either_side(ctx, kind, width):
    img = block_size_image(kind, width)
    stream, z, kinds = cpu_core(img)
    print("block sizes, %s %d: block kinds %s, %d -> %d bytes, ratio %.4f" % (kind, width, kinds, len(stream), len(z), len(z) / len(stream)))
    assert len(stream) == width + 1 and kinds == BLOCK_KINDS[(kind, width)]
    check_carriers(ctx, [img])


@pytest.mark.parametrize("nbytes", [262143, 832039])
def test_code_length_limit_and_kraft_repair_on_the_device_team(ctx, nbytes):
    """Fibonacci symbol counts: the unrestricted Huffman tree is deeper than 15, so the 256-thread team has to limit the lengths and repair the Kraft sum.
    One block exactly (262143 values + the filter byte) and the whole run (four blocks)."""
    img = carrier(fibonacci_values()[:nbytes])
    stream, z, kinds = cpu_core(img)
    assert stream[0] == 0                                              # "none": the block holds the values themselves
    ll, dist = U.dynamic_block_code_lengths(z)
    print("code-length limit, %d bytes: block kinds %s, %d -> %d bytes, ratio %.4f, %d literal/length codes of 15 bits, longest %d"
          % (nbytes, kinds, len(stream), len(z), len(z) / len(stream), ll.count(15), max(ll)))
    assert max(ll) == 15 and ll.count(15) > 2
    check_carriers(ctx, [img])


def test_long_repeats_of_a_sentence(ctx):
    img = carrier(b"the quick brown fox jumps over the lazy dog. " * 3000)
    stream, z, kinds = cpu_core(img)
    print("long repeats: block kinds %s, %d -> %d bytes, ratio %.4f" % (kinds, len(stream), len(z), len(z) / len(stream)))
    # the period of 45 bytes is far inside the window: behind the first period everything is matches, and their mean length is above 200 of the 258 possible
    assert kinds == (0, 0, 1) and cpu_tokens(img) < 46 + (len(stream) - 46) / 200
    check_carriers(ctx, [img])


@pytest.mark.parametrize("strength", [0, 19])
def test_identical_neighbours_in_one_group(ctx, strength):
    """four copies of one image, then two of the far-match stream, in one batch: a candidate from the neighbouring image would match every position
    perfectly.  Every stream must be that of the single-image call and of the CPU core."""
    a, c = P.synth_rgba(200, 150, 0, 3), tiled_chunk(32768, 262144 + 5000)
    arrays = [a, a.copy(), a.copy(), a.copy(), c, c.copy()]
    core = functools.lru_cache(maxsize=None)(U.deflate_host)            # (the one-row image has the same stream in both modes)
    for want_filters in (True, False):
        emitted, streams = run_both(ctx, arrays, strength, 2, want_filters)
        for group in (arrays[:4], arrays[4:]):
            e1, s1 = run_both(ctx, group[:1], strength, 2, want_filters)
            want, stats = core(stream_of(e1[0]))
            assert s1[0][1] == want and s1[0][2] == tuple(int(x) for x in stats[:3])
            if strength == 0 and group[0] is c:
                assert (stream_of(e1[0]), want) == cpu_core(c)[:2]
            for i, b in enumerate(arrays):
                if b.shape == group[0].shape:
                    assert stream_of(emitted[i]) == stream_of(e1[0]) and zlib.decompress(streams[i][1]) == stream_of(e1[0]), (i, want_filters)
                    assert streams[i] == s1[0], (i, want_filters)


def test_hundreds_of_images_shorter_than_a_key(ctx):
    """300 images of 1x1, 2x1, 1x2, 3x2 and 1x5 pixels in the four classes, in one batch: most positions have no key of their own and fall into the
    catch-all group that all images of the batch share"""
    rng = np.random.default_rng(43)
    shapes = [(1, 1), (2, 1), (1, 2), (3, 2), (1, 5)]
    classes = ("rgba", "rgb", "graya", "gray")
    arrays = [U.as_pixel_class(rng.integers(0, 4, (shapes[i % 5][1], shapes[i % 5][0], 4), dtype=np.uint8) * 85, classes[(i // 5) % 4]) for i in range(300)]
    for strength, want_filters in ((0, True), (0, False), (19, True), (19, False)):
        emitted, streams = run_both(ctx, arrays, strength, 2, want_filters)
        for i, (e, (ctype, z, blocks)) in enumerate(zip(emitted, streams)):
            want, stats = U.deflate_host(stream_of(e))
            assert ctype == e[0] and zlib.decompress(z) == stream_of(e), (i, strength, want_filters)
            assert z == want and blocks == tuple(int(x) for x in stats[:3]), (i, strength, want_filters)


CAMPAIGN_SEED, CAMPAIGN_BATCHES = 20261019, 40


def test_seeded_content_campaign(ctx):
    """tests/tools/gpu_deflate_fuzz.py with a fixed seed and a fixed number of batches: random shapes (the big ones capped at 400x300), the eight kinds of
    content of tests.util.deflate_fuzz_content, strengths 0 .. 255, both row_filters modes, batches of one to six images.  Colour type, inflate ==
    emitted, stream == CPU core.  40 batches are 133 images and take 1.7 s on an MI355X, most of it the CPU core."""
    rng = np.random.default_rng(CAMPAIGN_SEED)
    kinds, strengths, modes, images = set(), set(), set(), 0
    for _ in range(CAMPAIGN_BATCHES):
        arrays = []
        for _ in range(int(rng.integers(1, 7))):
            big = rng.random() < 0.15
            h = int(rng.integers(1, 300 if big else 60))
            w = int(rng.integers(1, 400 if big else 120))
            a, kind = U.deflate_fuzz_content(rng, h, w)
            arrays.append(a); kinds.add(kind)
        s = int(rng.choice([0, 5, 19, 40, 85, 255]))
        b = int(rng.choice([1, 2, 8, 32767]))
        wf = bool(rng.integers(0, 2))
        strengths.add(s); modes.add(wf)
        emitted, streams = run_both(ctx, arrays, s, b, wf)
        for i, (e, (ctype, z, blocks)) in enumerate(zip(emitted, streams)):
            data = stream_of(e)
            what = (images + i, arrays[i].shape, s, b, wf)
            assert ctype == e[0], what
            assert zlib.decompress(z) == data, what
            assert z == U.deflate_host(data)[0], what
        images += len(arrays)
    assert kinds == set(range(8)) and strengths == {0, 5, 19, 40, 85, 255} and modes == {True, False}, (kinds, strengths, modes)

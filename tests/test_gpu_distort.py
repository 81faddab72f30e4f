"""GPU tests of the distortion report: pngloss_hip_compare_batch on shapes the optimiser cannot produce, in a call of 260 pairs (8 workgroups per
image: long lane loops, a lane that flushes its 32-bit sums) and in one of 65 540 (a second launch), the option "distortion" on every optimise
entry point (outputs unchanged, records equal to numpy on original and output), the multi-device wrapper and the command line switch.

Every expected record comes from numpy on the two pixel arrays (tests/util_distort.py:np_distortion), the optimised pixels from the CPU oracle
(U.run_port); equality is exact, PSNR only appears in the tool's text, formatted by the same formula in Python."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D

pytestmark = pytest.mark.gpu

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
ZERO = dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _compare(ctx, pairs):
    """pairs of (H, W, 4) arrays through compare_batch; returns record dicts"""
    dev = [(_dev(a), _dev(b)) for a, b in pairs]
    recs = ctx.compare([(da.data_ptr(), db.data_ptr(), a.shape[1], a.shape[0]) for (da, db), (a, _) in zip(dev, pairs)])
    return [r.as_dict() for r in recs]


@functools.lru_cache(maxsize=None)
def _synth_and_port(w, h, mode, frame, s, b):
    img = P.synth_rgba(w, h, mode, frame)
    out, filt = U.run_port(img, s, b)
    for a in (img, out, filt):
        a.setflags(write=False)
    return img, out, filt


def _run_device(ctx, imgs, s, b, asynchronous=False):
    """a device-resident batch; returns (outs, filters, results)"""
    import torch
    dev = [_dev(a) for a in imgs]
    flt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
    desc = [(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)]
    if asynchronous:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        ctx.enqueue(desc, s, b, stream=st.cuda_stream)
        res = ctx.finish()
        st.synchronize()
    else:
        res = ctx.run(desc, s, b)
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dev], [f.cpu().numpy() for f in flt], res


def _check_device_case(cases, s, b, asynchronous=False):
    """cases: (w, h, mode, frame).  One batch with the option off and one with it on: same bytes, equal to the oracle's; records equal to numpy's."""
    ref = [_synth_and_port(w, h, m, fr, s, b) for (w, h, m, fr) in cases]
    imgs = [r[0] for r in ref]
    ctx = P.HipContext()
    try:
        off = _run_device(ctx, imgs, s, b, asynchronous)
        with pytest.raises(RuntimeError):
            ctx.distortion(0)                       # the batch ran with the option off
        ctx.set_option("distortion", "on")
        on = _run_device(ctx, imgs, s, b, asynchronous)
        recs = [ctx.distortion(i).as_dict() for i in range(len(imgs))]
        with pytest.raises(RuntimeError):
            ctx.distortion(len(imgs))
    finally:
        ctx.close()
    for i, (img, want, wf) in enumerate(ref):
        assert on[2][i]["status"] == 0 and off[2][i]["status"] == 0
        assert np.array_equal(on[0][i], off[0][i]) and np.array_equal(on[1][i], off[1][i]), cases[i]
        assert np.array_equal(on[0][i], want) and np.array_equal(on[1][i], wf), cases[i]
        assert recs[i] == D.np_distortion(img, want), cases[i]
    return recs, on[2]


# ------------------------------------------------------------------------------------------------ compare_batch

def test_compare_mixed_sizes_in_one_call():
    pairs = D.mixed_pairs()
    ctx = P.HipContext()
    try:
        got = _compare(ctx, pairs)
        assert ctx.compare([]) == []
    finally:
        ctx.close()
    for (a, b), g in zip(pairs, got):
        assert g == D.np_distortion(a, b), a.shape
    assert got[-1] == ZERO and pairs[-1][0].size == 0


def test_compare_bases_off_16_byte_alignment():
    import torch
    a, b = D.mixed_pairs()[4]
    assert a.shape == (5, 257, 4)
    want = D.np_distortion(a, b)
    n = a.size
    big_a, big_b = torch.zeros(n + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert big_a.data_ptr() % 16 == 0 and big_b.data_ptr() % 16 == 0
    ctx = P.HipContext()
    try:
        for oa, ob in ((4, 0), (0, 4), (4, 4)):
            va, vb = big_a[oa:oa + n], big_b[ob:ob + n]
            va.copy_(torch.from_numpy(a.reshape(-1))); vb.copy_(torch.from_numpy(b.reshape(-1)))
            torch.cuda.synchronize()
            assert va.data_ptr() % 16 == oa and vb.data_ptr() % 16 == ob
            got = ctx.compare([(va.data_ptr(), vb.data_ptr(), 257, 5)])[0].as_dict()
            assert got == want, (oa, ob)
    finally:
        ctx.close()


def test_compare_large_frames_sums_beyond_32_bits_and_a_single_last_pixel():
    import torch
    n = 2048 * 2048
    zeros = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    ones = torch.full((n * 4,), 255, dtype=torch.uint8, device="cuda")
    last = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    last[-1] = 1                                                   # the last pixel's alpha, + 1
    torch.cuda.synchronize()
    ctx = P.HipContext()
    try:
        full, one, same = [r.as_dict() for r in ctx.compare([(zeros.data_ptr(), ones.data_ptr(), 2048, 2048), (zeros.data_ptr(), last.data_ptr(), 2048, 2048),
                                                             (ones.data_ptr(), ones.data_ptr(), 2048, 2048)])]
    finally:
        ctx.close()
    # 2048 * 2048 * 255^2 = 272 734 617 600 per channel: beyond 2^32
    assert full == dict(pixels=n, changed_pixels=n, sq_err=[n * 255 * 255] * 4, max_abs=[255] * 4) and n * 255 * 255 == 272734617600 > 1 << 32
    assert one == dict(pixels=n, changed_pixels=1, sq_err=[0, 0, 0, 1], max_abs=[0, 0, 0, 1])
    assert same == dict(pixels=n, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)


#: the pair that makes a lane of pl_distort empty its 32-bit sums: 8192 x 4100 = 2048 lanes x 4100 quads.  With 256 or more pairs in a call an image has
#: 8 workgroups = 2048 lanes (D.grid_blocks) -- the fewest the rule gives -- and a lane flushes after D.FLUSH_PIXELS = 16 384 pixels, so this is the
#: smallest shape that reaches pld_flush inside the loops on a device: every lane flushes once, at its 4096th quad, and carries 4 quads to the end.
FLUSH_W, FLUSH_H, FLUSH_BLOCK_H = 8192, 4100, 100
#: pixel index -> the channel that gets the error, and the error: the very first pixel, lane 7's first quad after its flush, the very last pixel
FLUSH_MARKS = {0: (0, 255), 4 * (2048 * 4096 + 7): (2, 253), FLUSH_W * FLUSH_H - 1: (1, 254)}


@functools.lru_cache(maxsize=None)
def _flush_block():
    """a random 8192 x 100 pair (3.3 MB each), about half of its pixels changed, by at most 100 per channel"""
    rng = np.random.default_rng(17)
    a = rng.integers(0, 256, (FLUSH_BLOCK_H, FLUSH_W, 4), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-100, 101, a.shape) * (rng.random(a.shape[:2]) < 0.5)[..., None], 0, 255).astype(np.uint8)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def _flush_expected():
    """the record of the block repeated 41 times with the three marked pixels: 41 x numpy's record of the block, corrected for the three"""
    a, b = _flush_block()
    blk = D.np_distortion(a, b)
    reps = FLUSH_H // FLUSH_BLOCK_H
    assert reps * FLUSH_BLOCK_H == FLUSH_H and reps == 41 and max(blk["max_abs"]) <= 100 and 0 < blk["changed_pixels"] < blk["pixels"]
    rec = dict(pixels=reps * blk["pixels"], changed_pixels=reps * blk["changed_pixels"], sq_err=[reps * s for s in blk["sq_err"]], max_abs=list(blk["max_abs"]))
    fa, fb = a.reshape(-1, 4).astype(np.int64), b.reshape(-1, 4).astype(np.int64)
    for p, (c, err) in FLUSH_MARKS.items():
        was = fb[p % len(fa)] - fa[p % len(fa)]               # what the pixel under the mark added
        rec["changed_pixels"] += 1 - int(was.any())
        for k in range(4):
            rec["sq_err"][k] += (err * err if k == c else 0) - int(was[k]) ** 2
        rec["max_abs"][c] = err
    return rec


def _flush_build(view_a, view_b):
    """the pair into two device byte views of 8192 * 4100 * 4 bytes: the block 41 times, then the marks (a = 0, b = the error in one channel)"""
    import torch
    a, b = _flush_block()
    for view, blk in ((view_a, a), (view_b, b)):
        view.view(FLUSH_H // FLUSH_BLOCK_H, -1).copy_(torch.from_numpy(np.array(blk).reshape(1, -1)).cuda())
    for p, (c, err) in FLUSH_MARKS.items():
        view_a[4 * p: 4 * p + 4] = 0
        view_b[4 * p: 4 * p + 4] = 0
        view_b[4 * p + c] = err
    torch.cuda.synchronize()


def test_compare_260_pairs_small_grid_long_lane_loops_and_the_flush():
    """With 256 or more pairs in a call an image gets 8 workgroups, whatever its size: the grid-stride loops of pl_distort run long, as they do in
    production.  The flush pair (above), a 1021 x 517 noise pair -- some 64 quads per lane and a tail of one word -- from aligned bases and from
    bases 4 bytes off (every pixel through the word loop), and the mixed shapes over and over.  Then the same with the flush pair 4 bytes off
    alignment: 16 400 words per lane, the flush falls in the word loop.  Alone the flush pair has 2048 workgroups, no lane flushes: the same record."""
    import torch
    n, px = 260, FLUSH_W * FLUSH_H
    rng = np.random.default_rng(19)
    noise = tuple(rng.integers(0, 256, (517, 1021, 4), dtype=np.uint8) for _ in range(2))
    mixed = D.mixed_pairs()
    # the preconditions, from the restated grid rule alone
    assert n <= D.MAX_IMAGES and D.grid_blocks(n, px) == 8 and px == 33587200 == 8 * D.THREADS * 4 * 4100
    assert D.lane_pixels(n, px, px) == D.lane_pixels(n, px, px, vector=False) == 16400 > D.FLUSH_PIXELS > 16400 // 2      # one flush in the loop, 16 pixels after it
    assert D.lane_pixels(n, px, 1021 * 517) == 4 * 65 and 1021 * 517 % 4 == 1 and D.lane_pixels(n, px, 1021 * 517, vector=False) == 258
    assert D.lane_pixels(1, px, px) == 68 < D.FLUSH_PIXELS and D.grid_blocks(1, px) == 2048
    want_flush, want_noise, want_mixed = _flush_expected(), D.np_distortion(*noise), [D.np_distortion(a, b) for a, b in mixed]
    assert want_flush["max_abs"][:3] == [255, 254, 253] and want_flush["pixels"] == px and min(want_flush["sq_err"]) > 1 << 32
    big = [torch.empty(px * 4 + 16, dtype=torch.uint8, device="cuda") for _ in range(2)]
    off4 = [torch.zeros(noise[0].size + 16, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for t, x in zip(off4, noise):
        t[4: 4 + x.size].copy_(torch.from_numpy(x.reshape(-1)))
    dev_noise = [_dev(x) for x in noise]
    dev_mixed = [(_dev(a), _dev(b)) for a, b in mixed]
    assert all(t.data_ptr() % 16 == 0 for t in big + off4 + dev_noise)
    order = [k % len(mixed) for k in range(n - 3)]
    rest = [(dev_noise[0].data_ptr(), dev_noise[1].data_ptr(), 1021, 517), (off4[0].data_ptr() + 4, off4[1].data_ptr() + 4, 1021, 517)]
    rest += [(dev_mixed[k][0].data_ptr() if mixed[k][0].size else 0, dev_mixed[k][1].data_ptr() if mixed[k][0].size else 0) + mixed[k][0].shape[1::-1] for k in order]
    ctx = P.HipContext()
    try:
        for off in (0, 4):
            _flush_build(big[0][off: off + px * 4], big[1][off: off + px * 4])
            flush = (big[0].data_ptr() + off, big[1].data_ptr() + off, FLUSH_W, FLUSH_H)
            got = [r.as_dict() for r in ctx.compare([flush] + rest)]
            alone = ctx.compare([flush])[0].as_dict()
            print(off, got[0], alone)
            assert got[0] == want_flush, off
            assert alone == want_flush, off
            assert got[1] == want_noise and got[2] == want_noise, off
            for i, k in enumerate(order):
                assert got[3 + i] == want_mixed[k], (off, 3 + i, mixed[k][0].shape)
    finally:
        ctx.close()


def test_compare_more_pairs_than_one_launch_takes():
    """65 540 pairs: a launch takes 65 535 (D.MAX_IMAGES), so the last five are a second launch, which must start at its own jobs"""
    from tests import util_visible as V
    pool = V.split_pool()
    n = V.SPLIT_N
    assert n > D.MAX_IMAGES == 65535 and n - D.MAX_IMAGES < len(pool) == 7
    want = D.dicts_array([D.np_distortion(a, b) for _, a, b in pool])
    assert len({w.tobytes() for w in want}) == 7 and want["pixels"].tolist() == [1, 3, 64, 144, 117, 128, 0]
    dev = [(_dev(a), _dev(b)) for _, a, b in pool]
    desc = [(da.data_ptr() if a.size else 0, db.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for (da, db), (_, a, _) in zip(dev, pool)]
    ctx = P.HipContext()
    try:
        got = D.records_array(ctx.compare([desc[i % 7] for i in range(n)]))
    finally:
        ctx.close()
    bad = D.differing(got, want[np.arange(n) % 7])
    assert not bad.size, "%d records differ, the first at %s; around the end of the first launch: %s" % (
        bad.size, bad[:8].tolist(), {i: (got[i].tolist(), want[i % 7].tolist()) for i in range(65534, 65540)})


def test_compare_identical_pair_and_a_batch_in_flight():
    img = P.synth_rgba(160, 48, 0, 1)
    ctx = P.HipContext()
    try:
        assert _compare(ctx, [(img, img.copy())])[0] == dict(pixels=160 * 48, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)
        import torch
        d, f = _dev(img), torch.zeros(48, dtype=torch.uint8, device="cuda")
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), 160, 48)], 19, 2)
        out = (P.Distortion * 1)()
        pair = (P.lib.ImagePair * 1)(P.lib.ImagePair(d.data_ptr(), d.data_ptr(), 160, 48))
        assert P.hip_lib().pngloss_hip_compare_batch(ctx._ctx, pair, 1, out, None) == P.lib.PNGLOSS_INVALID_ARGUMENT
        assert P.hip_lib().pngloss_hip_last_distortion(ctx._ctx, 0, out) == P.lib.PNGLOSS_INVALID_ARGUMENT
        ctx.finish()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the optimise path with the option on

@pytest.mark.parametrize("w,h,mode", [(160, 48, 0), (160, 48, 2), (160, 48, 3), (160, 48, 4), (160, 48, 5), (1536, 24, 0)])
def test_option_on_every_class_and_both_engines(w, h, mode):
    recs, res = _check_device_case([(w, h, mode, 1)], 19, 2)
    assert recs[0]["pixels"] == w * h and recs[0]["changed_pixels"] > 0
    img = P.synth_rgba(w, h, mode, 1)
    gray, opaque = bool((img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()), bool((img[..., 3] == 255).all())
    assert res[0]["bpp"] == ((1 if opaque else 2) if gray else (3 if opaque else 4))
    assert {2: 3, 3: 2, 4: 1}.get(mode, 4) == res[0]["bpp"]            # the six cases cover the four classes


def test_option_on_the_smoke_batch():
    frames = [_synth_and_port(1536, 20, m, 3 + i, 19, 2) for i, m in enumerate((0, 0, 1, 0, 5, 0, 2, 0))]
    imgs = [f[0] for f in frames]
    ctx = P.HipContext()
    try:
        off = ctx.run_host(imgs, 19, 2)
        ctx.set_option("distortion", "on")
        on = ctx.run_host(imgs, 19, 2)
        recs = [ctx.distortion(i).as_dict() for i in range(len(imgs))]
    finally:
        ctx.close()
    for i, (img, want, wf) in enumerate(frames):
        assert on[2][i]["status"] == 0
        assert np.array_equal(on[0][i], off[0][i]) and np.array_equal(on[1][i], off[1][i])
        assert np.array_equal(on[0][i], want) and np.array_equal(on[1][i], wf)
        assert recs[i] == D.np_distortion(img, want), i


@pytest.mark.parametrize("w,h", [(160, 48), (1536, 24)])
def test_option_on_strength_0_changes_nothing(w, h):
    recs, _ = _check_device_case([(w, h, 0, 1)], 0, 2)
    assert recs[0] == dict(pixels=w * h, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)


def test_option_on_asynchronous_entry_on_a_stream_of_the_callers():
    _check_device_case([(160, 48, 0, 2), (1536, 24, 0, 2), (33, 7, 5, 2)], 19, 2, asynchronous=True)


def test_option_on_host_window_split_across_peers(monkeypatch):
    monkeypatch.setenv("PNGLOSS_HIP_SPLIT", "2")
    shapes = [(64, 48, 0), (130, 9, 2), (96, 64, 3), (33, 77, 4), (120, 50, 5), (257, 3, 1)]
    ref = [_synth_and_port(w, h, m, i, 19, 2) for i, (w, h, m) in enumerate(shapes)]
    imgs = [r[0] for r in ref]
    ctx = P.HipContext()
    try:
        ctx.set_option("distortion", "on")
        outs, filts, res = ctx.run_host(imgs, 19, 2)
        recs = [ctx.distortion(i).as_dict() for i in range(len(imgs))]
        engines = [ctx.engine_info(i) for i in range(len(imgs))]
        with pytest.raises(RuntimeError):
            ctx.distortion(len(imgs))
    finally:
        ctx.close()
    assert len(engines) == 6
    wants = [D.np_distortion(img, want) for img, want, _ in ref]
    assert len({(w["pixels"], tuple(w["sq_err"])) for w in wants}) == 6          # distinct images: a wrong chunk mapping shows
    for i, (img, want, wf) in enumerate(ref):
        assert res[i]["status"] == 0 and np.array_equal(outs[i], want) and np.array_equal(filts[i], wf)
        assert recs[i] == wants[i], i


def test_option_on_stream_only_zlib():
    shapes = [(160, 48, 0), (130, 9, 2), (96, 64, 4), (120, 50, 5)]
    ref = [_synth_and_port(w, h, m, 4, 19, 2) for (w, h, m) in shapes]
    imgs = [r[0] for r in ref]
    ctx = P.HipContext()
    try:
        _, _, z_off = ctx.run_host_zlib(imgs, 19, 2, stream_only=True)
        ctx.set_option("distortion", "on")
        ctx.run_host(imgs, 19, 2)
        plain = [ctx.distortion(i).as_dict() for i in range(len(imgs))]
        outs, _, z_on = ctx.run_host_zlib(imgs, 19, 2, stream_only=True)
        recs = [ctx.distortion(i).as_dict() for i in range(len(imgs))]
    finally:
        ctx.close()
    for i, (img, want, _) in enumerate(ref):
        assert np.array_equal(outs[i], img)                     # the host arrays are as they were
        assert z_on[i] == z_off[i] and len(z_on[i][1]) > 0
        assert recs[i] == plain[i] == D.np_distortion(img, want), i


def test_option_off_and_unknown_values():
    img = P.synth_rgba(64, 48, 0, 0)
    lib = P.hip_lib()
    ctx = P.HipContext()
    try:
        out = P.Distortion()
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == P.lib.PNGLOSS_INVALID_ARGUMENT        # no batch yet
        ctx.run_host([img], 19, 2)
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == P.lib.PNGLOSS_INVALID_ARGUMENT        # the option is off by default
        assert lib.pngloss_hip_set_option(ctx._ctx, b"distortion", b"maybe") == P.lib.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"distortion", b"") == P.lib.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"distortion", b"on") == 0
        ctx.run_host([img], 19, 2)
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == 0 and out.pixels == 64 * 48
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 1, out) == P.lib.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, None) == P.lib.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"distortion", b"off") == 0
        ctx.run_host([img], 19, 2)
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == P.lib.PNGLOSS_INVALID_ARGUMENT
    finally:
        ctx.close()


def test_multi_records_follow_the_images():
    shapes = [(64, 48, 0), (130, 9, 2), (96, 64, 3), (120, 50, 5)]
    ref = [_synth_and_port(w, h, m, i, 19, 2) for i, (w, h, m) in enumerate(shapes)]
    imgs = [r[0] for r in ref]
    multi = P.HipMulti("0,0")
    try:
        assert multi.count == 2
        with pytest.raises(RuntimeError):
            multi.set_option("distortion", "maybe")
        multi.set_option("distortion", "on")
        outs, filts, res = multi.run_host(imgs, 19, 2)
        recs = [multi.distortion(i).as_dict() for i in range(len(imgs))]
        with pytest.raises(RuntimeError):
            multi.distortion(len(imgs))
    finally:
        multi.close()
    assert sorted(P.multi_split([(w, h) for w, h, _ in shapes], 2)) == [0, 0, 1, 1]          # both contexts got images
    for i, (img, want, wf) in enumerate(ref):
        assert res[i]["status"] == 0 and np.array_equal(outs[i], want) and np.array_equal(filts[i], wf)
        assert recs[i] == D.np_distortion(img, want), i


# ------------------------------------------------------------------------------------------------ the tool

@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers on this box)")
def test_tool_prints_one_line_per_written_file_and_writes_the_same_files(tmp_path):
    from PIL import Image
    png, inputs = U.load_npz("suite_png.npz"), U.load_npz("suite_inputs.npz")
    names = ["david", "tux"]
    s, b = 25, 3
    ctx = P.HipContext()
    try:
        outs, _, res = ctx.run_host([inputs[n] for n in names], s, b)
    finally:
        ctx.close()
    want_lines = [D.cli_line(D.np_distortion(inputs[n], o), r["bpp"]) for n, o, r in zip(names, outs, res)]
    assert all("PSNR" in line for line in want_lines)
    written, stderr = {}, {}
    for tag, args in (("plain", []), ("plain+d", ["--distortion"]), ("gpu", ["--gpu-read", "--gpu-deflate"]), ("gpu+d", ["--gpu-read", "--gpu-deflate", "--distortion"])):
        d = tmp_path / tag
        d.mkdir()
        for n in names:
            (d / f"{n}.png").write_bytes(png[n].tobytes())
        r = subprocess.run([OUR_CLI, "-s", str(s), "-b", str(b)] + args + [str(d / f"{n}.png") for n in names], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stderr[-800:])
        written[tag] = [(d / f"{n}-loss.png").read_bytes() for n in names]
        stderr[tag] = r.stderr.splitlines()
    assert written["plain"] == written["plain+d"] and written["gpu"] == written["gpu+d"]
    for tag in ("plain", "gpu"):
        assert not [x for x in stderr[tag] if "distortion" in x]
        assert [x for x in stderr[tag + "+d"] if x.startswith("  distortion:")] == want_lines, (tag, stderr[tag + "+d"])
        assert [x for x in stderr[tag + "+d"] if not x.startswith("  distortion:")] == stderr[tag]      # nothing else on stderr moves
    for n, o, data in zip(names, outs, written["plain"]):
        import io
        assert np.array_equal(np.array(Image.open(io.BytesIO(data)).convert("RGBA")), o), n
    # the verbose run keeps its lines and gets the new one behind "writing compressed image", in file order
    d = tmp_path / "verbose"
    d.mkdir()
    (d / "david.png").write_bytes(png["david"].tobytes())
    r = subprocess.run([OUR_CLI, "-v", "--distortion", "-s", str(s), "-b", str(b), str(d / "david.png")], capture_output=True, text=True, timeout=300)
    lines = r.stderr.splitlines()
    assert r.returncode == 0 and want_lines[0] in lines and lines.index(want_lines[0]) > [i for i, x in enumerate(lines) if "writing compressed image" in x][0]
    # strength 0 changes no pixel: the other form of the line
    d = tmp_path / "lossless"
    d.mkdir()
    (d / "david.png").write_bytes(png["david"].tobytes())
    r = subprocess.run([OUR_CLI, "--distortion", "-s", "0", str(d / "david.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [x for x in r.stderr.splitlines() if "distortion" in x] == ["  distortion: none (lossless)"]

"""GPU parity tests (-m gpu): the HIP path, called through the C ABI of libpngloss_hip.so, against
  (a) the committed golden fixtures produced by the real reference,
  (b) the CPU oracle on seeded inputs,
  (c) the reference digests of the full-size BASELINE.json configurations, and size-independent properties.
Bar: bit-exact pixels and filter IDs (integer/byte work, no tolerance)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(params=["seg", "wg", "lead"])
def engine_choice(request, monkeypatch):
    """The library has two row engines and picks per batch: few large images -> the SEGMENT-PARALLEL engine (one image over the whole
    GPU, pl_seg.hip), batches -> one workgroup per image (pl_engine.hip), which in turn picks, row by row, between its band-leader
    chains and its round-1 chains.  The tests that care pin each: "seg" the segment engine, "wg" the workgroup engine with its own
    adaptive choice, "lead" the workgroup engine with the band-leader chains pinned (the library reads the variable on every call)."""
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", request.param)
    return request.param


def test_extension_is_loaded_and_sees_the_gpu():
    lib = P.hip_lib()
    assert lib.pngloss_hip_device_count() >= 1
    assert b"gfx950" in lib.pngloss_hip_version()


@pytest.mark.parametrize("case", U.SYNTH_CASES, ids=U.case_key)
def test_golden_synthetic(case):
    w, h, m, s, b, fr, filt = case
    g = U.load_npz("synth_cases.npz")
    out, f = P.optimize_with_rows(P.synth_rgba(w, h, m, fr), s, b, want_filters=filt)
    assert np.array_equal(out, g[U.case_key(case) + "/out"])
    if filt:
        assert np.array_equal(f, g[U.case_key(case) + "/filters"])


@pytest.mark.parametrize("name", ["rose", "david", "tux"])
def test_golden_suite_images(name):
    g = U.load_npz("suite_small.npz")
    out, f = P.optimize_with_rows(g[name + "/in"], 19, 2)
    assert np.array_equal(out, g[name + "/out"])
    assert np.array_equal(f, g[name + "/filters"])


def test_seeded_inputs_against_oracle():
    for img, s, b, filt in U.seeded_cases(seed=7, n=48):
        o1, f1 = U.run_port(img, s, b, filt)
        o2, f2 = P.optimize_with_rows(img, s, b, want_filters=filt)
        assert np.array_equal(o1, o2), (img.shape, s, b, filt)
        if filt:
            assert np.array_equal(f1, f2), (img.shape, s, b, filt)


@pytest.mark.parametrize("strength", [0, 1, 7, 8, 15, 16, 19, 20, 23, 24, 31, 32, 33, 40, 47, 48, 63, 64, 79, 80, 85, 95, 96, 127, 128, 255])
def test_every_candidate_count_path(strength):
    """s<=15: one candidate per lane, s<=31: two, above: the generic sweep -- each against the oracle, every class."""
    for mode in (0, 1, 3, 4, 5):
        img = P.synth_rgba(70, 10, mode, strength)
        o1, f1 = U.run_port(img, strength, 2)
        o2, f2 = P.optimize_with_rows(img, strength, 2)
        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (strength, mode)


@pytest.mark.parametrize("bleed", [1, 2, 3, 7, 8, 100, 32767])
def test_bleed_dividers(bleed):
    for mode in (0, 1, 5):
        img = P.synth_rgba(66, 12, mode, bleed)
        o1, f1 = U.run_port(img, 40, bleed)
        o2, f2 = P.optimize_with_rows(img, 40, bleed)
        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (bleed, mode)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 1), (1, 7), (63, 2), (64, 2), (65, 3), (128, 2), (129, 2), (300, 1)])
def test_edge_shapes_both_modes(shape):
    w, h = shape
    for mode in (1, 0, 3, 4, 5):
        for filt in (True, False):
            img = P.synth_rgba(w, h, mode, 0)
            o1, f1 = U.run_port(img, 19, 2, filt)
            o2, f2 = P.optimize_with_rows(img, 19, 2, want_filters=filt)
            assert np.array_equal(o1, o2), (shape, mode, filt)
            if filt:
                assert np.array_equal(f1, f2), (shape, mode, filt)


def test_empty_image_is_a_no_op():
    out, f = P.optimize_with_rows(np.zeros((0, 0, 4), np.uint8), 19, 2)
    assert out.size == 0 and f.size == 0
    out, f = P.optimize_with_rows(np.zeros((3, 0, 4), np.uint8), 19, 2)
    assert out.shape == (3, 0, 4)


def test_strength_zero_identity_and_determinism():
    for mode in range(6):
        img = P.synth_rgba(200, 40, mode, 9)
        out, f = P.optimize_with_rows(img, 0, 2)
        assert np.array_equal(out, img)
    img = P.synth_rgba(333, 77, 0, 4)
    a = P.optimize_with_rows(img, 19, 2)
    b = P.optimize_with_rows(img, 19, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_legacy_entry_points():
    """optimize_with_stride / optimizeForAverageFilter (pngloss_image.c:29-50): row_filters = NULL mode."""
    img = P.synth_rgba(90, 30, 0, 1)
    want, _ = U.run_port(img, 25, 2, filters=False)
    assert np.array_equal(P.optimize_for_average_filter(img, 25), want)
    want8, _ = U.run_port(img, 25, 8, filters=False)
    assert np.array_equal(P.optimize_with_stride(img, 25, 8), want8)


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_optimize_image_lower_seam(bpp):
    """optimize_image (pngloss_image.h:26-29) on packed data, no gray/alpha detection: e.g. an RGB image whose
    pixels happen to be gray must still be treated as 3 B/px."""
    rng = np.random.default_rng(bpp)
    packed = rng.integers(0, 256, (14, 37, bpp), dtype=np.uint8)
    if bpp in (2, 4):
        packed[rng.random((14, 37)) < 0.2, bpp - 1] = 0
    if bpp == 3:
        packed[...] = packed[..., :1]
    o1, f1 = U.run_port_packed(packed, 19, 2)
    o2, f2 = P.optimize_image(packed, 19, 2)
    assert np.array_equal(o1, o2) and np.array_equal(f1, f2)
    o1, _ = U.run_port_packed(packed, 19, 2, filters=False)
    o2, _ = P.optimize_image(packed, 19, 2, want_filters=False)
    assert np.array_equal(o1, o2)


def test_invalid_arguments_are_rejected():
    img = P.synth_rgba(8, 8, 0, 0)
    with pytest.raises(RuntimeError):
        P.optimize_with_rows(img, 19, 0)
    with pytest.raises(RuntimeError):
        P.optimize_with_rows(img, 19, 40000)


def test_device_resident_batch_of_mixed_images(torch_cuda):
    """The batched extension: 9 images of all classes and sizes in one launch, device pointers from torch."""
    torch = torch_cuda
    specs = [(64, 48, 0), (70, 46, 2), (180, 215, 4), (33, 9, 3), (265, 31, 5), (1, 1, 1), (129, 65, 1), (5, 1, 0), (96, 64, 4)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
    ctx = P.HipContext()
    res = ctx.run([(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], 19, 2,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_bpp = {0: 4, 1: 4, 2: 3, 3: 2, 4: 1, 5: 4}
    for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
        o1, f1 = U.run_port(a, 19, 2)
        assert np.array_equal(d.cpu().numpy(), o1), specs[i]
        assert np.array_equal(f.cpu().numpy(), f1), specs[i]
        assert r["status"] == 0 and r["bpp"] == want_bpp[specs[i][2]]
        # final histogram: one symbol per channel byte, and the unique-symbol count of pngloss_image.c:311-325
        h, w = a.shape[:2]
        hist = ctx.histogram(i)
        assert int(hist.sum()) == w * h * r["bpp"]
        assert int((hist != 0).sum()) == r["unique_symbols"]
    assert ctx.engine_ms > 0 and ctx.total_ms >= ctx.engine_ms
    ctx.close()


def test_strength_retry_rows_are_reported(torch_cuda):
    """pngloss_image.c:266-274: smooth gray input needs the strength-decrement retry on the adaptive first row; with
    row_filters == NULL every row is adaptive and many rows retry.  The HIP path must agree with the oracle's trace."""
    import ctypes as C
    torch = torch_cuda
    img = P.synth_rgba(96, 64, 4, 0)
    h, w = img.shape[:2]
    packed = np.ascontiguousarray(img[..., 1:2])
    for want_filters in (True, False):
        out = packed.copy()
        f = np.zeros(h, np.uint8)
        su = np.zeros(h, np.uint8)
        tr = U.PortTrace(None, su.ctypes.data, None, None)
        assert U.port().port_optimize_packed(out.ctypes.data, w, h, 1, f.ctypes.data if want_filters else None, 19, 2, C.byref(tr)) == 0
        want_retried = int((su < 19).sum())
        d = torch.from_numpy(img.copy()).cuda()
        df = torch.zeros(h, dtype=torch.uint8, device="cuda")
        ctx = P.HipContext()
        res = ctx.run([(d.data_ptr(), df.data_ptr() if want_filters else 0, w, h)], 19, 2)
        assert res[0]["retried_rows"] == want_retried and want_retried >= 1
        assert np.array_equal(d.cpu().numpy()[..., 1:2], out)
        ctx.close()


@pytest.mark.parametrize("engine", ["seg", "wg"])
@pytest.mark.parametrize("shift_words", [1, 2, 3])
def test_device_pointers_need_only_pixel_alignment(torch_cuda, monkeypatch, engine, shift_words):
    """the device-resident entry point takes whatever RGBA8 pointer the caller has: a frame that starts 4, 8 or 12 bytes behind a 16-byte
    boundary (a view into a larger buffer) must give the reference's result -- the kernels' 16-byte loads are an optimisation, not a contract"""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", engine)
    w, h = 256, 48
    a = P.synth_rgba(w, h, 0, 7)
    big = torch.zeros(w * h + 8, dtype=torch.int32, device="cuda")
    view = big[shift_words:shift_words + w * h]
    view.copy_(torch.from_numpy(a.view(np.int32).reshape(-1)).cuda())
    f = torch.zeros(h, dtype=torch.uint8, device="cuda")
    ctx = P.HipContext()
    ctx.run([(view.data_ptr(), f.data_ptr(), w, h)], 19, 2)
    want, want_f = U.run_port(a, 19, 2)
    got = view.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(f.cpu().numpy(), want_f)
    assert int(big[:shift_words].abs().sum()) == 0 and int(big[shift_words + w * h:].abs().sum()) == 0     # nothing written outside the frame
    ctx.close()


@pytest.mark.gpu
def test_seam_takes_rows_that_are_not_contiguous():
    """optimize_with_rows (pngloss_image.h:21-25) gets an array of row pointers; the caller's rows need not be contiguous, ordered or
    evenly spaced: rows placed backwards in a buffer with an odd stride, and a stride-based call with padding
    behind every row -- both against the oracle, and the bytes between the rows untouched"""
    import ctypes as C
    w, h = 150, 37
    a = P.synth_rgba(w, h, 0, 11)
    want, want_f = U.run_port(a, 19, 2)
    stride = w * 4 + 20
    buf = np.full(h * stride + 64, 0xA5, np.uint8)
    rows = (C.c_void_p * h)()
    for y in range(h):
        off = 8 + (h - 1 - y) * stride                      # row y sits in front of row y - 1
        buf[off:off + w * 4] = a[y].reshape(-1)
        rows[y] = buf.ctypes.data + off
    filt = np.zeros(h, np.uint8)
    rc = P.hip_lib().optimize_with_rows(rows, w, h, filt.ctypes.data_as(C.c_void_p), False, 19, 2)
    assert rc == 0
    for y in range(h):
        off = 8 + (h - 1 - y) * stride
        assert np.array_equal(buf[off:off + w * 4].reshape(w, 4), want[y]), y
        assert (buf[off + w * 4:off + stride] == 0xA5).all()
    assert np.array_equal(filt, want_f)
    # optimize_with_stride: the same frame with 12 bytes of padding behind every row (row_filters = NULL mode)
    want_n, _ = U.run_port(a, 19, 2, filters=False)
    stride2 = w * 4 + 12
    buf2 = np.full(h * stride2, 0x5A, np.uint8)
    for y in range(h):
        buf2[y * stride2:y * stride2 + w * 4] = a[y].reshape(-1)
    P.hip_lib().optimize_with_stride(buf2.ctypes.data_as(C.c_void_p), w, h, stride2, False, 19, 2)
    for y in range(h):
        assert np.array_equal(buf2[y * stride2:y * stride2 + w * 4].reshape(w, 4), want_n[y]), y
        assert (buf2[y * stride2 + w * 4:(y + 1) * stride2] == 0x5A).all()


def test_batch_histogram_matches_oracle(torch_cuda):
    torch = torch_cuda
    a = P.synth_rgba(150, 40, 2, 3)
    d = torch.from_numpy(a.copy()).cuda()
    f = torch.zeros(40, dtype=torch.uint8, device="cuda")
    ctx = P.HipContext()
    ctx.run([(d.data_ptr(), f.data_ptr(), 150, 40)], 30, 2)
    _, _, hist = U.run_port_packed(np.ascontiguousarray(a[..., :3]), 30, 2, trace=True)
    assert np.array_equal(ctx.histogram(0), hist)
    ctx.close()


@pytest.mark.parametrize("width", [152, 150, 4, 8, 260])
@pytest.mark.parametrize("mode", [0, 2, 3, 4])
def test_original_histogram_every_class_and_both_loaders(torch_cuda, width, mode):
    """pl_hist (optimize_state.c:66-83) counts four pixels per thread when a row is a whole number of 16-byte quads and pixel by
    pixel otherwise; every bytes-per-pixel class (generator modes 0, 2, 3, 4 -> 4, 3, 2, 1) through both, against the oracle."""
    torch = torch_cuda
    h = 37
    a = P.synth_rgba(width, h, mode, 5)
    d = torch.from_numpy(a.copy()).cuda()
    f = torch.zeros(h, dtype=torch.uint8, device="cuda")
    ctx = P.HipContext()
    ctx.run([(d.data_ptr(), f.data_ptr(), width, h)], 19, 2)
    bpp = {0: 4, 2: 3, 3: 2, 4: 1}[mode]
    packed = {4: a, 3: a[..., :3], 2: a[..., [1, 3]], 1: a[..., 1:2]}[bpp]
    want, want_f, hist = U.run_port_packed(np.ascontiguousarray(packed), 19, 2, trace=True)
    got = d.cpu().numpy()
    got_packed = {4: got, 3: got[..., :3], 2: got[..., [1, 3]], 1: got[..., 1:2]}[bpp]
    assert np.array_equal(got_packed, want)
    assert np.array_equal(f.cpu().numpy(), want_f)
    assert np.array_equal(ctx.histogram(0), hist)       # (the running histogram after the last row: every tie was broken alike)
    ctx.close()


def test_reference_digests_1080p_frames():
    for e in U.load_digests()["synthetic"]:
        if (e["width"], e["height"]) != (1920, 1080):
            continue
        out, f = P.optimize_with_rows(P.synth_rgba(1920, 1080, 0, e["frame"]), 19, 2)
        assert "%016x" % P.fnv1a64(out, P.SURVEY_FNV_BASIS) == e["out"], e
        assert "%016x" % P.fnv1a64(f, P.SURVEY_FNV_BASIS) == e["filters"], e


def test_reference_digest_headline_4096(torch_cuda, engine_choice):
    """BASELINE.json configs[1]: 4096x4096 synthetic RGBA8, s=19, b=2 -- digests measured on the real reference (with the
    kernel's adaptive choice of chains, and with the band-leader chains pinned)."""
    e = [e for e in U.load_digests()["synthetic"] if e["width"] == 4096][0]
    img = P.synth_rgba(4096, 4096, 0, 0)
    assert "%016x" % P.fnv1a64(img, P.SURVEY_FNV_BASIS) == e["in"]
    out, f = P.optimize_with_rows(img, 19, 2)
    assert "%016x" % P.fnv1a64(out, P.SURVEY_FNV_BASIS) == e["out"]
    assert "%016x" % P.fnv1a64(f, P.SURVEY_FNV_BASIS) == e["filters"]
    # size-independent properties at full size: only the five legal filter flags, alpha never leaves [224,255]
    assert set(np.unique(f)) <= set(P.PNG_FILTER_FLAGS)
    assert int(np.abs(out.astype(np.int16) - img.astype(np.int16)).max()) <= 2 * 19 + 8


def test_suite_batch_all_eleven_images_match_reference_digests(torch_cuda):
    """BASELINE.json configs[2]: the reference's eleven suite images (decoded RGBA8 inputs in tests/golden/suite_inputs.npz)
    as ONE image-parallel batch through the device-resident API; every output and filter list must match the digests the
    real reference produced (tests/golden/digests.json, /root/reference/suite/*.png at s=19 b=2)."""
    torch = torch_cuda
    inputs = np.load(os.path.join(U.GOLDEN, "suite_inputs.npz"))
    digests = {e["image"]: e for e in U.load_digests()["suite"]}
    names = sorted(inputs.files)
    assert len(names) == 11 and set(names) == set(digests)
    imgs = [inputs[n] for n in names]
    for n, a in zip(names, imgs):
        assert "%016x" % P.fnv1a64(a, P.SURVEY_FNV_BASIS) == digests[n]["in"], n
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
    ctx = P.HipContext()
    res = ctx.run([(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], 19, 2,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_bpp = dict(barbara=1, david=1, dice=4, girl=3, lena=3, parrots=3, redbrush=4, rose=3, ssr=1, tenko=3, tux=4)
    for n, d, f, r in zip(names, dev, filt, res):
        assert r["status"] == 0 and r["bpp"] == want_bpp[n], (n, r)
        assert "%016x" % P.fnv1a64(d.cpu().numpy(), P.SURVEY_FNV_BASIS) == digests[n]["out"], n
        assert "%016x" % P.fnv1a64(f.cpu().numpy(), P.SURVEY_FNV_BASIS) == digests[n]["filters"], n
    ctx.close()


def test_strength_bleed_sweep_8192_matches_reference_digests(torch_cuda):
    """BASELINE.json configs[4]: strength {0,20,40,85} x bleed {1,2,8} on the 8192x8192 frame, the twelve points run
    concurrently (one workgroup = one CU each); outputs and filter lists against the reference-measured digests of
    SURVEY.md Appendix B (tests/golden/digests.json)."""
    torch = torch_cuda
    dig = U.load_digests()["synthetic"]
    base = P.synth_rgba(8192, 8192, 0, 0)
    points = [(s, b) for s in (0, 20, 40, 85) for b in (1, 2, 8)]
    ctxs = [P.HipContext() for _ in points]
    streams = [torch.cuda.Stream() for _ in points]
    dev = [torch.from_numpy(base).cuda() for _ in points]
    filt = [torch.zeros(8192, dtype=torch.uint8, device="cuda") for _ in points]
    torch.cuda.synchronize()
    for c, st, d, f, (s, b) in zip(ctxs, streams, dev, filt, points):
        c.enqueue([(d.data_ptr(), f.data_ptr(), 8192, 8192)], s, b, stream=st.cuda_stream)
    for c in ctxs:
        c.finish()
    torch.cuda.synchronize()
    for c, d, f, (s, b) in zip(ctxs, dev, filt, points):
        e = [e for e in dig if e["width"] == 8192 and e["strength"] == s and (e["bleed"] == b or s == 0)][0]
        if not os.environ.get("PNGLOSS_HIP_ENGINE"):
            assert c.engine_info(0)["engine"] == ("row-statistics (strength 0)" if s == 0 else "segment-parallel"), (s, b, c.engine_info(0))    # every point of configs[4] is on a fast engine
        assert "%016x" % P.fnv1a64(d.cpu().numpy(), P.SURVEY_FNV_BASIS) == e["out"], (s, b)
        assert "%016x" % P.fnv1a64(f.cpu().numpy(), P.SURVEY_FNV_BASIS) == e["filters"], (s, b)
        c.close()


def test_segment_engine_is_the_default_for_single_images_and_reports_what_it_did(torch_cuda):
    """No engine pinned: a single wide image goes through the segment engine whatever the strength (engine_info says so: state sets
    beyond the lanes are enumerated from seeds), narrow images go to the workgroup engine; all exact."""
    torch = torch_cuda
    env_before = os.environ.pop("PNGLOSS_HIP_ENGINE", None)
    try:
        # (a narrow image is faster on the workgroup engine: the segment engine's row attempt costs the same whatever the width)
        for (w, s, b, want) in [(1000, 19, 2, "segment-parallel"), (1000, 85, 2, "segment-parallel"), (1000, 255, 1, "segment-parallel"), (200, 19, 2, "workgroup-per-image")]:
            img = P.synth_rgba(w, 70, 0, 4)
            d = torch.from_numpy(img.copy()).cuda()
            f = torch.zeros(70, dtype=torch.uint8, device="cuda")
            ctx = P.HipContext()
            res = ctx.run([(d.data_ptr(), f.data_ptr(), w, 70)], s, b, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            info = ctx.engine_info(0)
            assert info["engine"] == want, info
            if want == "segment-parallel":
                assert info["attempts"] >= 70 and info["serial_rows"] == 0 and info["walked_segments"] <= 250   # (s = 255: the seeds miss the reference's own state in ~0.2 % of the segments)
            o1, f1 = U.run_port(img, s, b)
            assert res[0]["status"] == 0 and np.array_equal(d.cpu().numpy(), o1) and np.array_equal(f.cpu().numpy(), f1)
            ctx.close()
    finally:
        if env_before is not None:
            os.environ["PNGLOSS_HIP_ENGINE"] = env_before


def test_segment_engine_batch_of_mixed_images(torch_cuda, monkeypatch):
    """Several images of different sizes and classes in ONE segment-engine batch (blockIdx.y = image; images finish at different
    attempts, incl. a 1x1 one that is done at once), rows that need the strength retry, NULL row_filters."""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    specs = [(300, 40, 0), (1, 1, 1), (64, 48, 4), (700, 25, 5), (33, 77, 3), (129, 10, 2), (512, 16, 1)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") if i != 3 else None for i, a in enumerate(imgs)]
    ctx = P.HipContext()
    res = ctx.run([(d.data_ptr(), f.data_ptr() if f is not None else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], 19, 2,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
        assert ctx.engine_info(i)["engine"] == "segment-parallel"
        o1, f1 = U.run_port(a, 19, 2, filters=f is not None)
        assert r["status"] == 0 and np.array_equal(d.cpu().numpy(), o1), (i, specs[i])
        if f is not None:
            assert np.array_equal(f.cpu().numpy(), f1), (i, specs[i])
    ctx.close()


def test_strength_zero_row_engine_matches_oracle_and_the_other_engines(torch_cuda, monkeypatch):
    """Strength 0 has a row engine of its own (pl_rows.hip: nothing is quantised, so the row's residual counts do not depend on earlier rows; one parallel pass
    for the counts, one serial pass over the rows for the decisions).  Against the oracle and against the segment and workgroup engines pinned: every
    byte-per-pixel class, both row_filters modes (every row adaptive / row 0 only), ragged and tiny shapes, a batch of mixed images, bleed irrelevant;
    the engine reports itself; at strength 1 the library does not pick it."""
    torch = torch_cuda
    monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    specs = [(300, 40, 0), (1, 1, 1), (64, 48, 4), (700, 25, 5), (33, 77, 3), (129, 10, 2), (512, 16, 1), (2, 3, 0), (1, 9, 2), (1537, 5, 0)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    for with_filters in (True, False):
        want = [U.run_port(a, 0, 2, filters=with_filters) for a in imgs]
        # the histogram after the last row depends on every row's decision: it makes the decisions of the NULL mode observable
        want_hist = []
        for a in imgs:
            gray, opaque = bool((a[..., 0] == a[..., 1]).all() and (a[..., 1] == a[..., 2]).all()), bool((a[..., 3] == 255).all())
            packed = (a[..., 1:2] if opaque else a[..., [1, 3]]) if gray else (a[..., :3] if opaque else a)
            want_hist.append(U.run_port_packed(np.ascontiguousarray(packed), 0, 2, filters=with_filters, trace=True)[2])
        for eng in (None, "seg", "wg"):
            if eng: monkeypatch.setenv("PNGLOSS_HIP_ENGINE", eng)
            else: monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
            ctx = P.HipContext()
            dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
            filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") if with_filters else None for a in imgs]
            res = ctx.run([(d.data_ptr(), f.data_ptr() if f is not None else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], 0, 7)
            torch.cuda.synchronize()
            for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
                assert r["status"] == 0 and np.array_equal(d.cpu().numpy(), want[i][0]) and np.array_equal(d.cpu().numpy(), a), (eng, with_filters, i)
                if f is not None:
                    assert np.array_equal(f.cpu().numpy(), want[i][1]), (eng, with_filters, i, specs[i])
                if eng is None:
                    assert ctx.engine_info(i)["engine"] == "row-statistics (strength 0)"
                assert np.array_equal(ctx.histogram(i), want_hist[i]), (eng, with_filters, i, specs[i])
                assert r["unique_symbols"] == int(np.count_nonzero(want_hist[i])), (eng, with_filters, i, specs[i])
            ctx.close()
    monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    ctx = P.HipContext()
    d = torch.from_numpy(imgs[0].copy()).cuda(); f = torch.zeros(imgs[0].shape[0], dtype=torch.uint8, device="cuda")
    ctx.run([(d.data_ptr(), f.data_ptr(), 300, 40)], 1, 2)
    assert ctx.engine_info(0)["engine"] != "row-statistics (strength 0)"
    ctx.close()


def test_synchronous_and_asynchronous_entry_points_agree(torch_cuda, monkeypatch):
    """pngloss_hip_optimize_batch (no device-side wait on the caller's stream, three launch groups for a batch in units) against pngloss_hip_optimize_batch_async +
    pngloss_hip_finish (stream wait, two groups) on the same inputs: a batch of 14 frames of 1920 x 40 (units: > 680 segments), a mixed small batch and a single
    image, on a side stream with work enqueued behind the call; both against the oracle; contexts created and destroyed in between (the engine's streams are
    taken from and returned to the process-wide list)."""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    st = torch.cuda.Stream()
    for specs in ([(1920, 40, 0)] * 14, [(300, 40, 0), (200, 90, 1), (64, 48, 4)], [(1536, 24, 5)]):
        imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
        want = [U.run_port(a, 19, 2) for a in imgs]
        for mode in ("sync", "async", "sync"):
            ctx = P.HipContext()
            dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
            filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
            torch.cuda.synchronize()
            desc = [(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)]
            with torch.cuda.stream(st):
                if mode == "sync":
                    res = ctx.run(desc, 19, 2, stream=st.cuda_stream)
                else:
                    ctx.enqueue(desc, 19, 2, stream=st.cuda_stream)
                copies = [d.clone() for d in dev]              # enqueued behind the call on the same stream: must see the optimised pixels
                if mode == "async":
                    res = ctx.finish()
            st.synchronize()
            for i, (d, f, c, r) in enumerate(zip(dev, filt, copies, res)):
                assert r["status"] == 0 and np.array_equal(d.cpu().numpy(), want[i][0]) and np.array_equal(f.cpu().numpy(), want[i][1]), (mode, i)
                assert np.array_equal(c.cpu().numpy(), want[i][0]), ("work behind the call ran ahead of the engine", mode, i)
            ctx.close()


@pytest.mark.parametrize("groups", [None, "1", "2"])
def test_segment_engine_launch_groups_of_small_and_mixed_batches(torch_cuda, monkeypatch, groups):
    """Round 5: a batch of two or more images runs as TWO launch sequences on two streams (pl_host.hip:run_seg_engine) -- the tallest image alone when it stands
    out, equal shares otherwise; the library sorts the segment engine's images by height for that.  Results must not depend on it: the library's own choice,
    one group and two equal groups (PNGLOSS_HIP_SEG_GROUPS) all give the oracle's bytes, image by image in the caller's order -- heights in every order, ties,
    a 1x1 image, NULL row_filters, and the same context used for a second batch of another shape."""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    if groups is not None:
        monkeypatch.setenv("PNGLOSS_HIP_SEG_GROUPS", groups)
    ctx = P.HipContext()
    for specs in ([(300, 40, 0), (200, 90, 1), (64, 48, 4), (700, 25, 5), (33, 77, 3), (1, 1, 1), (512, 90, 2)],      # tallest in the middle, a tie for the tallest
                  [(260, 30, 2), (180, 64, 0)],                                                                    # two images: one each
                  [(640, 20, 1), (640, 20, 3), (640, 20, 5)],                                                      # equal heights: equal shares
                  [(96, 120, 0), (400, 16, 4), (300, 16, 1), (50, 16, 2)]):                                        # one image far taller than the rest
        imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
        dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
        filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") if i != 1 else None for i, a in enumerate(imgs)]
        res = ctx.run([(d.data_ptr(), f.data_ptr() if f is not None else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], 19, 2,
                      stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
            assert ctx.engine_info(i)["engine"] == "segment-parallel"
            o1, f1 = U.run_port(a, 19, 2, filters=f is not None)
            assert r["status"] == 0 and np.array_equal(d.cpu().numpy(), o1), (groups, i, specs[i])
            if f is not None:
                assert np.array_equal(f.cpu().numpy(), f1), (groups, i, specs[i])
    ctx.close()


def test_engine_choice_on_batches_of_1080p_frames(torch_cuda, monkeypatch):
    """Which row engine the library picks for n frames of 1920x1080 in one batch (no engine pinned): the segment engine up to ~148 such frames
    (round 6, units from seeds: 128 frames 325 ms against 373; round 5: 116), one workgroup per image beyond -- and the bytes do not depend
    on it: frames 0 and n-1 against the other engine's output of the same frames."""
    torch = torch_cuda
    monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    base = [P.synth_rgba(1920, 1080, 0, i) for i in range(2)]
    ref = None
    for n, want in [(136, "segment-parallel"), (164, "workgroup-per-image")]:
        ctx = P.HipContext()
        dev = [torch.from_numpy(base[i % 2].copy()).cuda() for i in range(n)]
        filt = [torch.zeros(1080, dtype=torch.uint8, device="cuda") for _ in range(n)]
        res = ctx.run([(d.data_ptr(), f.data_ptr(), 1920, 1080) for d, f in zip(dev, filt)], 19, 2, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert all(r["status"] == 0 for r in res)
        assert ctx.engine_info(0)["engine"] == want and ctx.engine_info(n - 1)["engine"] == want, (n, ctx.engine_info(0))
        got = [(dev[i].cpu().numpy(), filt[i].cpu().numpy()) for i in (0, n - 1)]       # frame n-1 is generator frame 1 for both n
        if ref is None:
            ref = got
        else:
            for (o, f), (o2, f2) in zip(ref, got):
                assert np.array_equal(o, o2) and np.array_equal(f, f2)
        ctx.close()
        del dev, filt


def test_segment_engine_strengths_and_bleeds_with_few_and_many_states(monkeypatch):
    """(strength, bleed) pairs from one chain state (s = 0) to the most the lanes hold; widths around the segment (32), group (512)
    and commit-workgroup (1024) sizes; every byte-per-pixel class."""
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    for (w, h, m, s, b) in [(31, 9, 0, 19, 2), (32, 9, 1, 19, 2), (33, 9, 2, 19, 2), (511, 7, 3, 19, 2), (513, 7, 4, 19, 2), (1025, 6, 5, 19, 2),
                            (200, 30, 0, 0, 2), (200, 30, 1, 3, 1), (200, 30, 5, 7, 3), (200, 30, 0, 20, 8), (200, 30, 2, 19, 4), (200, 30, 1, 19, 32767), (200, 30, 0, 30, 3),
                            # state sets enumerated in several chunks of lanes (259 .. 955 states), rows whose segments have more distinct
                            # states than the chain kernel's usual table stride
                            (1100, 12, 0, 20, 2), (1100, 12, 1, 20, 1), (700, 16, 2, 40, 2), (1100, 12, 0, 85, 8), (520, 16, 4, 26, 2), (300, 16, 3, 40, 2)]:
        img = P.synth_rgba(w, h, m, 2)
        o1, f1 = U.run_port(img, s, b)
        o2, f2 = P.optimize_with_rows(img, s, b)
        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (w, h, m, s, b)


@pytest.mark.parametrize("nt", ["512", "1024"])
def test_segment_engine_both_sizes_of_the_enumeration_workgroups(monkeypatch, nt):
    """the enumeration's workgroups have 512 threads (a channel pair) for narrow rows / few images and 1024 beyond; PNGLOSS_HIP_ENUM_NT pins one"""
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    monkeypatch.setenv("PNGLOSS_HIP_ENUM_NT", nt)
    ctx = P.HipContext()                   # (the timing / test hooks of the environment are read when a context is created -- round 6 --, so: a context of this test's own)
    for (w, h, m, s, b) in [(700, 20, 0, 19, 2), (1100, 12, 1, 20, 1), (513, 9, 4, 19, 2), (300, 16, 3, 40, 2), (3300, 6, 0, 19, 2), (200, 30, 5, 7, 3)]:
        img = P.synth_rgba(w, h, m, 2)
        o1, f1 = U.run_port(img, s, b)
        (o2,), (f2,), res = ctx.run_host([img], s, b)
        assert res[0]["status"] == 0 and ctx.engine_info(0)["engine"] == "segment-parallel"
        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (w, h, m, s, b)
    ctx.close()


def test_both_chain_kinds_of_the_workgroup_engine_in_one_image(torch_cuda, monkeypatch):
    """PNGLOSS_HIP_ENGINE=mix: band-leader chains and round-1 chains take turns every four rows, whatever the cycle counters say
    (the adaptive choice of the default mode depends on timing and would not reproduce a mismatch of either kind); the engine
    reports how many rows each kind took, results are the oracle's."""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "mix")
    for (w, h, m, s, b) in [(300, 64, 0, 19, 2), (200, 48, 5, 19, 2), (130, 40, 3, 40, 1), (96, 40, 1, 7, 3)]:
        img = P.synth_rgba(w, h, m, 3)
        d = torch.from_numpy(img.copy()).cuda()
        f = torch.zeros(h, dtype=torch.uint8, device="cuda")
        ctx = P.HipContext()
        res = ctx.run([(d.data_ptr(), f.data_ptr(), w, h)], s, b, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        info = ctx.engine_info(0)
        o1, f1 = U.run_port(img, s, b)
        assert res[0]["status"] == 0 and np.array_equal(d.cpu().numpy(), o1) and np.array_equal(f.cpu().numpy(), f1), (w, h, m, s, b)
        assert info["engine"] == "workgroup-per-image"
        assert info["attempts"] >= h // 4 and info["serial_rows"] >= h // 4, info      # band-leader row attempts, rows on the round-1 chains
        ctx.close()


def test_round1_chains_still_match_the_oracle():
    """The round-1 chain formulation stays in the kernel for rows the band-leader chains do not take (q > 128, large incoming
    errors); PNGLOSS_HIP_ENGINE=legacy runs every row through it.  Checked in a fresh process (the hook is read per call)."""
    code = ("import os, sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import pngloss_amd as P\n"
            "from tests import util as U\n"
            "for (w, h, m, s, b) in [(96, 40, 0, 19, 2), (130, 33, 5, 40, 1), (64, 48, 3, 85, 8), (200, 20, 1, 7, 3)]:\n"
            "    img = P.synth_rgba(w, h, m, 2)\n"
            "    o1, f1 = U.run_port(img, s, b)\n"
            "    o2, f2 = P.optimize_with_rows(img, s, b)\n"
            "    assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (w, h, m, s, b)\n"
            "print('legacy ok')\n") % U.ROOT
    env = dict(os.environ, PNGLOSS_HIP_ENGINE="legacy")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "legacy ok" in r.stdout, r.stderr[-1500:]


_commit_capacity_refs = {}


def _commit_capacity_case(width, kind, filters):
    """image and the oracle's answer, worked out once per case and shared by the engines"""
    key = (width, kind, filters)
    if key not in _commit_capacity_refs:
        h = 4
        if kind == "rgba noise":
            img = np.random.default_rng(width).integers(0, 256, (h, width, 4), dtype=np.uint8)
        else:
            x = np.arange(width, dtype=np.int64)[None, :] + 37 * np.arange(h, dtype=np.int64)[:, None]
            img = np.zeros((h, width, 4), np.uint8)
            img[..., 1] = (x * 255 // (width + 37 * h)).astype(np.uint8)
            img[..., 3] = (255 - x * 200 // (width + 37 * h)).astype(np.uint8)
            img = U.as_pixel_class(img, "graya")
        out, filt = U.run_port(img, 19, 2, filters=filters)
        for a in (img, out) + ((filt,) if filters else ()):
            a.setflags(write=False)
        _commit_capacity_refs[key] = (img, out, filt)
    return _commit_capacity_refs[key]


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("engine", ["wg", "lead", "legacy"])
def test_workgroup_engine_rows_at_the_commit_capacity(monkeypatch, engine, over):
    """The commit pass of the workgroup engine keeps a row's next-rows terms in LDS where the row fits the union the chains leave free, 16 bytes a pixel, and
    takes the pass without LDS for wider rows: the widest row of the first kind and the narrowest of the second (the capacity read from the layout,
    pngloss_amd/csrc/pl_wg_lds.h, not written down here), both kinds of chains, four and two bytes a pixel, with and without row filters."""
    cap = U.wg_lds_layout()["commit_px"]
    assert cap * 16 <= U.wg_lds_layout()["union_bytes"] < (cap + 1) * 16
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", engine)
    for kind in ("rgba noise", "gray+alpha gradient"):
        for filters in (True, False):
            img, want, want_f = _commit_capacity_case(cap + over, kind, filters)
            out, filt = P.optimize_with_rows(img, 19, 2, want_filters=filters)
            assert np.array_equal(out, want), (engine, cap + over, kind, filters)
            assert (filt is None and want_f is None) if not filters else np.array_equal(filt, want_f), (engine, cap + over, kind, filters)


def test_band_leader_chains_on_hostile_inputs(engine_choice):
    """Inputs chosen against the band-leader chains: noise (every band in use, ties everywhere), values around 128 (filter
    none's positive and negative bands compete for the same bins), saturated and fully transparent regions (static and
    dynamic clamps, forced symbols), widths around the 64-pixel chunk, large strengths (few, wide bands)."""
    rng = np.random.default_rng(11)
    cases = []
    for (w, h) in [(63, 12), (64, 12), (65, 12), (257, 9), (300, 40)]:
        a = rng.integers(118, 140, (h, w, 4), dtype=np.uint8); a[..., 3] = 255
        cases.append((a, 19, 2))
        b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8); b[..., 3] = np.where(rng.random((h, w)) < 0.4, 0, b[..., 3])
        cases.append((b, 19, 2))
        c = np.full((h, w, 4), 255, np.uint8); c[:, ::7] = 0; c[h // 2:, :, :3] = rng.integers(230, 256, (h - h // 2, w, 3), dtype=np.uint8)
        cases.append((c, 30, 1))
    cases += [(P.synth_rgba(200, 30, m, 5), s, b) for m in range(6) for (s, b) in [(63, 2), (127, 1), (5, 8)]]
    for i, (img, s, b) in enumerate(cases):
        o1, f1 = U.run_port(img, s, b)
        o2, f2 = P.optimize_with_rows(img, s, b)
        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (i, img.shape, s, b)


def test_light_pixels_and_deferred_bumps_on_saturated_frames(engine_choice):
    """Saturated and nearly saturated regions: the clamp [lo, lo+255] cuts bands down to one value ("light" pixels, settled without
    reading the histogram, bumps deferred and checked at the next flush) or to a few (exact redo behind a flush), next to ordinary
    fast pixels.  Frames large enough for big histogram counts, so that the watched relations and their close-bin map matter;
    the oracle's band-leader variant must agree with its plain chain on the same frames (same decisions, proven on the CPU)."""
    rng = np.random.default_rng(23)
    frames = []
    for (w, h) in [(640, 96), (1000, 64)]:
        ramp = np.linspace(-40, 300, w)[None, :, None] + rng.normal(0, 9, (h, w, 4))           # black .. white with both ends clipped
        a = np.clip(ramp, 0, 255).astype(np.uint8); a[..., 3] = 255
        b = np.where(rng.random((h, w, 1)) < 0.35, 255, rng.integers(200, 256, (h, w, 4))).astype(np.uint8)   # white with texture
        c = np.where(rng.random((h, w, 1)) < 0.35, 0, rng.integers(0, 40, (h, w, 4))).astype(np.uint8)        # black with texture
        c[..., 3] = np.where(rng.random((h, w)) < 0.1, 0, 255)
        frames += [np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)]
    for i, img in enumerate(frames):
        for (s, b) in [(19, 2), (7, 1), (40, 4)]:
            o0, f0 = U.run_port(img, s, b, variant=0)
            o1, f1 = U.run_port(img, s, b, variant=2)
            assert np.array_equal(o0, o1) and np.array_equal(f0, f1), ("oracle variants disagree", i, s, b)
            o2, f2 = P.optimize_with_rows(img, s, b)
            assert np.array_equal(o0, o2) and np.array_equal(f0, f2), (i, img.shape, s, b)


def test_multi_device_host_batch_two_contexts_on_one_device():
    """The node-level C entry point (one context + host thread per device, LPT split, results in input order) with the device
    list "0,0": two contexts sharing the one GPU of this box exercise the split, the threads and the scatter."""
    specs = [(200, 150, 0), (64, 48, 2), (300, 20, 5), (1, 1, 1), (130, 90, 3), (96, 64, 4), (257, 33, 1)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    multi = P.HipMulti("0,0")
    assert multi.count == 2
    outs, filts, res = multi.run_host(imgs, 19, 2)
    multi.close()
    own = P.multi_split([(w, h) for (w, h, m) in specs], 2)
    assert set(own) == {0, 1}
    for a, o, f, r, sp in zip(imgs, outs, filts, res, specs):
        o1, f1 = U.run_port(a, 19, 2)
        assert r["status"] == 0 and np.array_equal(o, o1) and np.array_equal(f, f1), sp
    # the same through one context, and with the environment variable instead of the argument
    ctx = P.HipContext()
    outs1, filts1, _ = ctx.run_host(imgs, 19, 2)
    ctx.close()
    assert all(np.array_equal(x, y) for x, y in zip(outs, outs1)) and all(np.array_equal(x, y) for x, y in zip(filts, filts1))


def test_async_entry_returns_at_once_and_overlaps_host_work(torch_cuda, monkeypatch):
    """pngloss_hip_optimize_batch_async on the segment-parallel engine (whose number of launches depends on the data): the call returns
    in milliseconds -- a helper thread of the context feeds the attempts to the engine's own stream, the caller's stream waits for the
    device-written finished word --, host work between _async and _finish overlaps the GPU, a kernel the caller enqueues on its stream
    behind the call sees the finished image, and the blocking variant (devices without stream memory operations) gives the same bytes."""
    import time
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    w, h = 2048, 1024
    img = P.synth_rgba(w, h, 0, 0)
    want, wf = U.run_port(img, 19, 2)
    ctx = P.HipContext()
    st = torch.cuda.Stream()
    enq, fin = [], []
    for rep in range(3):
        d = torch.from_numpy(img.copy()).cuda()
        f = torch.zeros(h, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), w, h)], 19, 2, stream=st.cuda_stream)
        t1 = time.perf_counter()
        with torch.cuda.stream(st):
            behind = d.clone()                                # enqueued by the caller behind the batch, before _finish
        time.sleep(0.03)                                      # host work
        t2 = time.perf_counter()
        res = ctx.finish()
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        enq.append(t1 - t0); fin.append((t3 - t2, ctx.engine_ms * 1e-3))
        assert res[0]["status"] == 0 and ctx.engine_info(0)["engine"] == "segment-parallel"
        assert torch.equal(behind, d), "work enqueued on the caller's stream behind the call ran before the batch had finished"
        assert np.array_equal(d.cpu().numpy(), want) and np.array_equal(f.cpu().numpy(), wf)
    full = d.cpu().numpy()
    assert min(enq[1:]) < 0.005, enq                          # (the first call creates the stream and the thread; measured 0.3 ms afterwards)
    assert all(fw < eng - 0.015 for fw, eng in fin[1:]), fin  # _finish waited for less than the engine took: the 30 ms of host work overlapped
    ctx.close()
    monkeypatch.setenv("PNGLOSS_HIP_NO_STREAM_WAIT", "1")
    ctx = P.HipContext()
    d2 = torch.from_numpy(img.copy()).cuda()
    f2 = torch.zeros(h, dtype=torch.uint8, device="cuda")
    ctx.run([(d2.data_ptr(), f2.data_ptr(), w, h)], 19, 2, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), full) and np.array_equal(f2.cpu().numpy(), f.cpu().numpy())
    ctx.close()


def test_three_launch_groups_are_opt_in_and_do_not_slow_a_later_asynchronous_batch(tmp_path):
    """The advisor's finding on round 5: the synchronous entry point ran large batches as THREE launch groups by itself, and a third engine stream in the process
    halves every later engine run that waits on a caller's stream -- nothing stopped a process from doing both.  Round 6: three groups are opt-in
    (pngloss_hip_set_option "launch_groups" "3"), the default is two, and once a third engine stream exists the asynchronous entry takes its blocking variant.
    In ONE process (a subprocess of the test: the third stream would stay with the pytest process): an asynchronous batch with a stream of its own (timed),
    a synchronous batch by default (two groups) and one opted in (three), the asynchronous batch again -- same bytes throughout, the engine not slower than
    1.5x its first run, no device-side wait any more."""
    script = tmp_path / "groups.py"
    script.write_text(
        "import sys, time, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "import pngloss_amd as P\n"
        "from tests import util as U\n"
        "st = torch.cuda.Stream()\n"
        "w, h = 2048, 384\n"
        "img = P.synth_rgba(w, h, 0, 3)\n"
        "want, wf = U.run_port(img, 19, 2)\n"
        "def one_async(ctx):\n"
        "    best, info = 1e9, None\n"
        "    for rep in range(3):\n"
        "        d = torch.from_numpy(img.copy()).cuda(); f = torch.zeros(h, dtype=torch.uint8, device='cuda'); torch.cuda.synchronize()\n"
        "        ctx.enqueue([(d.data_ptr(), f.data_ptr(), w, h)], 19, 2, stream=st.cuda_stream)\n"
        "        res = ctx.finish(); torch.cuda.synchronize()\n"
        "        assert res[0]['status'] == 0 and np.array_equal(d.cpu().numpy(), want) and np.array_equal(f.cpu().numpy(), wf)\n"
        "        best = min(best, ctx.engine_ms); info = ctx.engine_info(0)\n"
        "    return best, info\n"
        "frames = [P.synth_rgba(1920, 40, 0, i) for i in range(16)]\n"
        "oracle = [U.run_port(a, 19, 2) for a in frames]\n"
        "def batch(ctx):\n"
        "    dev = [torch.from_numpy(a.copy()).cuda() for a in frames]; flt = [torch.zeros(40, dtype=torch.uint8, device='cuda') for _ in frames]\n"
        "    res = ctx.run([(d.data_ptr(), f.data_ptr(), 1920, 40) for d, f in zip(dev, flt)], 19, 2); torch.cuda.synchronize()\n"
        "    for d, f, r, (o, of) in zip(dev, flt, res, oracle):\n"
        "        assert r['status'] == 0 and np.array_equal(d.cpu().numpy(), o) and np.array_equal(f.cpu().numpy(), of)\n"
        "    return ctx.engine_info(0)\n"
        "import os; os.environ['PNGLOSS_HIP_ENGINE'] = 'seg'\n"
        "a = P.HipContext(); b = P.HipContext(); c = P.HipContext()\n"
        "t_before, i_before = one_async(a)\n"
        "g_default = batch(b)\n"
        "c.set_option('launch_groups', '3')\n"
        "g_three = batch(c)\n"
        "t_after, i_after = one_async(a)\n"
        "print('RESULT', t_before, t_after, i_before['stream_wait'], i_after['stream_wait'], g_default['launch_groups'], g_three['launch_groups'])\n"
        % U.ROOT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PNGLOSS_HIP_SEG_GROUPS", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    t_before, t_after, w_before, w_after, g_default, g_three = [float(x) for x in r.stdout.split("RESULT")[1].split()]
    assert g_default == 2 and w_before == 1
    # a process that had put a wait on a caller's stream gets no third engine stream even when it asks for one; in a process without such a wait the opt-in works
    assert g_three == 2, "a third engine stream was created in a process that uses stream waits"
    assert t_after < 1.5 * t_before, (t_before, t_after)
    script2 = tmp_path / "groups2.py"
    script2.write_text(script.read_text().replace("t_before, i_before = one_async(a)\n", "t_before, i_before = 0.0, dict(stream_wait=-1)\n"))
    r = subprocess.run([sys.executable, str(script2)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    t_before, t_after, w_before, w_after, g_default, g_three = [float(x) for x in r.stdout.split("RESULT")[1].split()]
    assert g_default == 2 and g_three == 3 and w_after == 0, (g_default, g_three, w_after)     # three groups on request; the asynchronous entry then waits on the host


def test_engine_cost_model_calibration_is_opt_in_and_changes_no_bytes(tmp_path):
    """Round 6: with PNGLOSS_HIP_CALIB=1 the first batch of two or more images whose engine is the library's to choose times a small synthetic frame on both row engines (a
    context of its own, ~30 ms, once per device and process) and scales the cost model by what it finds against the reference box (pl_host.hip:engine_calib).  It is OFF by
    default: measured inside bench.py, a probe of a few milliseconds reads the clock governor's mood as much as the box (profiles/r06_host_side.txt).  One process with the
    switch: the calibration line is printed once (PNGLOSS_HIP_DEBUG=1), both batches equal the oracle whatever it found; a process without it prints none."""
    script = tmp_path / "calib.py"
    script.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "import pngloss_amd as P\n"
        "from tests import util as U\n"
        "for rnd in range(2):\n"
        "    ctx = P.HipContext()\n"
        "    imgs = [P.synth_rgba(640, 40, m, rnd) for m in (0, 1, 5)]\n"
        "    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]; flt = [torch.zeros(40, dtype=torch.uint8, device='cuda') for _ in imgs]\n"
        "    res = ctx.run([(d.data_ptr(), f.data_ptr(), 640, 40) for d, f in zip(dev, flt)], 19, 2); torch.cuda.synchronize()\n"
        "    for a, d, f, r in zip(imgs, dev, flt, res):\n"
        "        o, of = U.run_port(a, 19, 2)\n"
        "        assert r['status'] == 0 and np.array_equal(d.cpu().numpy(), o) and np.array_equal(f.cpu().numpy(), of)\n"
        "    ctx.close()\n"
        "print('calib ok')\n" % U.ROOT)
    env = dict(os.environ, PNGLOSS_HIP_DEBUG="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PNGLOSS_HIP_ENGINE", None)
    env.pop("PNGLOSS_HIP_CALIB", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=dict(env, PNGLOSS_HIP_CALIB="1"))
    assert r.returncode == 0 and "calib ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stderr.splitlines() if "engine calibration" in ln]
    assert len(lines) == 1 and "256 CUs" in lines[0] and "cost model scales" in lines[0], lines
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "calib ok" in r.stdout and "engine calibration" not in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]


def test_segment_engine_from_two_contexts_and_two_ranks_at_once(torch_cuda, monkeypatch, tmp_path):
    """What one box can show of a node: the SEGMENT engine (pinned) from two contexts of the C host at once (device list "0,0": two launch
    threads, two engine streams, two 150 KB chain kernels interleaved on one device), and from two processes (gloo ranks, one HipContext
    each, frames of pngloss_amd.shard's split) -- digests against the oracle."""
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    imgs = [P.synth_rgba(2048, 256, m, i) for i, m in enumerate((0, 1, 0, 5))]
    multi = P.HipMulti("0,0")
    assert multi.count == 2
    outs, filts, res = multi.run_host(imgs, 19, 2)
    multi.close()
    for a, o, f, r in zip(imgs, outs, filts, res):
        o1, f1 = U.run_port(a, 19, 2)
        assert r["status"] == 0 and np.array_equal(o, o1) and np.array_equal(f, f1)
    # two ranks on the one device
    code = (
        "import os, sys, numpy as np, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r)\n"
        "import pngloss_amd as P\n"
        "from pngloss_amd import shard as S\n"
        "from tests import util as U\n"
        "rank = int(os.environ['RANK']); dist.init_process_group('gloo', rank=rank, world_size=2)\n"
        "os.environ['PNGLOSS_HIP_ENGINE'] = 'seg'\n"
        "mine = S.contiguous_partition(4, 2)[rank]\n"
        "frames = [P.synth_rgba(2048, 128, 0, i) for i in mine]\n"
        "dev = [torch.from_numpy(a.copy()).cuda() for a in frames]; flt = [torch.zeros(128, dtype=torch.uint8, device='cuda') for _ in frames]\n"
        "ctx = P.HipContext(0)\n"
        "dist.barrier()\n"
        "res = ctx.run([(d.data_ptr(), f.data_ptr(), 2048, 128) for d, f in zip(dev, flt)], 19, 2)\n"
        "assert all(r['status'] == 0 for r in res) and ctx.engine_info(0)['engine'] == 'segment-parallel'\n"
        "for a, d, f in zip(frames, dev, flt):\n"
        "    o1, f1 = U.run_port(a, 19, 2)\n"
        "    assert np.array_equal(d.cpu().numpy(), o1) and np.array_equal(f.cpu().numpy(), f1)\n"
        "recs = S.gather_records([dict(index=i) for i in mine])\n"
        "if rank == 0: assert sorted(r['index'] for r in recs) == [0, 1, 2, 3]; print('two ranks ok')\n"
        "dist.destroy_process_group()\n") % U.ROOT
    script = tmp_path / "two_ranks.py"
    script.write_text(code)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29579", str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "two ranks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_every_visible_device_takes_part_when_there_are_several(tmp_path):
    """The REAL multi-device branch (the "0,0" test above shares one GPU): with two or more visible devices, HipMulti(None) opens one
    context per device and every one must come back with its share, bit-exact; and a 2-rank bench.py under torch.distributed.run (RCCL)
    must print a line whose frames_per_gpu and digests are right.  Skipped, with the reason, on a one-GPU box -- so that the first
    multi-GPU box the driver gets runs a test, not a debugging session."""
    ndev = P.hip_lib().pngloss_hip_device_count()
    if ndev < 2:
        pytest.skip("only %d HIP device visible: the multi-device branch needs two (the split logic itself is covered with devices '0,0')" % ndev)
    specs = [(200 + 7 * i, 60 + 3 * i, i % 6) for i in range(4 * ndev)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    multi = P.HipMulti(None)
    assert multi.count == ndev
    outs, filts, res = multi.run_host(imgs, 19, 2)
    multi.close()
    assert set(P.multi_split([(w, h) for (w, h, m) in specs], ndev)) == set(range(ndev))
    for a, o, f, r, sp in zip(imgs, outs, filts, res, specs):
        o1, f1 = U.run_port(a, 19, 2)
        assert r["status"] == 0 and np.array_equal(o, o1) and np.array_equal(f, f1), sp
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PNGLOSS_HIP_ENGINE", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29577",
                        os.path.join(U.ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["bit_exact_vs_reference_digest"] is True
    assert line["batch"]["frames_per_gpu"] == [128, 128] and line["batch"]["digests_match_reference"] is True
    assert line["batch_saturating"]["digests_match_reference"] is True


def test_verbose_prints_progress_and_summary():
    """-v surface of the seam (pngloss_image.c:214-237, 309-325): a spinner with the percentage of finished rows while the
    engine runs, then "compression complete" and "used N unique symbols"; the pixels are the same as without it."""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import pngloss_amd as P\n"
            "img = P.synth_rgba(1920, 400, 0, 0)\n"
            "o1, f1 = P.optimize_with_rows(img, 19, 2)\n"
            "o2, f2 = P.optimize_with_rows(img, 19, 2, verbose=True)\n"
            "assert np.array_equal(o1, o2) and np.array_equal(f1, f2)\n"
            "print('verbose ok')\n") % U.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "verbose ok" in r.stdout, r.stderr[-1500:]
    assert "% complete" in r.stderr and "compression complete" in r.stderr and "unique symbols" in r.stderr, r.stderr[-800:]


def test_careful_int16_wrap_variant_of_the_chain():
    """Rows whose incoming Sierra error exceeds 8000 switch the chain to a variant with explicit int16 sign
    extensions.  Natural images never get there, so a test hook forces that variant for every row;
    it must give the same bytes.  Run in a subprocess because the hook is read from the environment per batch."""
    import os
    import subprocess
    import sys
    code = (
        "import numpy as np, pngloss_amd as P\n"
        "from tests import util as U\n"
        "for m in range(6):\n"
        "    for (s, b) in [(19, 2), (40, 1), (85, 8), (7, 3)]:\n"
        "        img = P.synth_rgba(150, 20, m, s)\n"
        "        o1, f1 = U.run_port(img, s, b)\n"
        "        o2, f2 = P.optimize_with_rows(img, s, b)\n"
        "        assert np.array_equal(o1, o2) and np.array_equal(f1, f2), (m, s, b)\n"
        "print('careful ok')\n")
    env = dict(os.environ, PNGLOSS_HIP_FORCE_CAREFUL="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=U.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "careful ok" in r.stdout, r.stderr[-1500:]


def test_emitted_png_scanlines(torch_cuda):
    """Write side, device part: colour type of the optimised pixels, per-row PNG filter types (heuristic on row 0 /
    on every row in NULL mode, the optimiser's choice elsewhere) and the filtered bytes -- against a numpy restatement
    applied to the ORACLE's output, for every class, ragged widths and both row_filters modes."""
    specs = [(64, 48, 0), (70, 46, 2), (33, 77, 4), (96, 20, 3), (120, 50, 5), (1, 1, 1), (5, 3, 0), (257, 9, 2), (130, 40, 1), (31, 31, 4)]
    imgs = [P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate(specs)]
    # an RGB image whose optimised version happens to be ... still RGB, plus a constant image (gray output from "rgba" input)
    imgs.append(np.full((9, 40, 4), 200, np.uint8))
    ctx = P.HipContext()
    for want_filters in (True, False):
        outs, filts, emitted = ctx.run_host_emit(imgs, 19, 2, want_filters=want_filters)
        for a, o, f, (ctype, ids, rows) in zip(imgs, outs, filts, emitted):
            o1, f1 = U.run_port(a, 19, 2, want_filters)
            assert np.array_equal(o, o1)
            want_ct, want_ids, want_rows = U.png_scanlines_reference(o1, f1 if want_filters else None)
            assert ctype == want_ct, (a.shape, ctype, want_ct)
            assert np.array_equal(ids, want_ids), (a.shape, want_filters)
            assert np.array_equal(rows, want_rows), (a.shape, want_filters)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key,s,b,filters", [("r4_many_attempts_s200_b32767_null", 200, 32767, False), ("r4_many_attempts_s255_b3_ids", 255, 3, True)])
def test_segment_engine_tiny_images_that_need_very_many_attempts(monkeypatch, key, s, b, filters):
    """the two cases of tests/test_seg_host.py::test_seg_engine_tiny_images_that_need_very_many_attempts through the C ABI on the device
    (the launch thread's bound on the attempts now counts the strength retries)"""
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    img = U.load_npz("fuzz_regressions.npz")[key]
    out, f = P.optimize_with_rows(img, s, b, want_filters=filters)
    want, wf = U.run_port(img, s, b, filters)
    assert np.array_equal(out, want) and (not filters or np.array_equal(f, wf))


@pytest.mark.gpu
def test_engine_option_of_the_abi_pins_the_row_engine(torch_cuda, monkeypatch):
    """pngloss_hip_set_option(ctx, "engine", ...) -- the ABI's switch for what PNGLOSS_HIP_ENGINE does for the tests: same bytes either way,
    pngloss_hip_last_engine_info says which engine ran; unknown names and values are refused."""
    torch = torch_cuda
    monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    img = P.synth_rgba(640, 96, 0, 2)
    want, wf = U.run_port(img, 19, 2)
    ctx = P.HipContext()
    seen = []
    for value in ("seg", "wg", "auto"):
        ctx.set_option("engine", value)
        d = torch.from_numpy(img.copy()).cuda()
        f = torch.zeros(img.shape[0], dtype=torch.uint8, device="cuda")
        res = ctx.run([(d.data_ptr(), f.data_ptr(), img.shape[1], img.shape[0])], 19, 2)
        torch.cuda.synchronize()
        assert res[0]["status"] == 0 and np.array_equal(d.cpu().numpy(), want) and np.array_equal(f.cpu().numpy(), wf), value
        seen.append(ctx.engine_info(0)["engine"])
    assert seen[0] == "segment-parallel" and seen[1] == "workgroup-per-image"
    lib = P.hip_lib()
    assert lib.pngloss_hip_set_option(ctx._ctx, b"engine", b"fastest") == 4 and lib.pngloss_hip_set_option(ctx._ctx, b"colour", b"seg") == 4
    ctx.close()


def test_segment_engine_workspace_binding_at_the_smallest_shapes(torch_cuda, monkeypatch):
    """The per-image workspace of the segment engine is bound to its job record through one table (pl_plan.h: pl_seg_layout, pl_seg_bind): the shapes at which a size or
    a binding can be wrong -- one segment, SEG_L pixels and one more, a second replay group, a width that is no multiple of anything -- in ONE batch with an empty image,
    which goes to the other engine (a mixed batch: the selection list is used), at a state set within the lanes and at a seeded one, which has no `maps`."""
    torch = torch_cuda
    monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    specs = [(1, 2, 1), (32, 3, 0), (33, 3, 5), (513, 3, 2), (700, 4, 0), (0, 0, 0)]
    imgs = [P.synth_rgba(w, h, m, i) if w else np.zeros((0, 0, 4), np.uint8) for i, (w, h, m) in enumerate(specs)]
    ctx = P.HipContext()
    ctx.set_option("engine", "seg")
    for s, b in [(19, 2), (85, 1)]:
        dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
        filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
        res = ctx.run([(d.data_ptr() if a.size else 0, f.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], s, b)
        torch.cuda.synchronize()
        for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
            assert r["status"] == 0, (s, b, specs[i], r)
            if not a.size:
                continue
            assert ctx.engine_info(i)["engine"] == "segment-parallel", (s, b, specs[i])
            want, wf = U.run_port(a, s, b)
            assert np.array_equal(d.cpu().numpy(), want) and np.array_equal(f.cpu().numpy(), wf), (s, b, specs[i])
    ctx.close()


@pytest.mark.parametrize("hooks", [dict(PNGLOSS_HIP_SEG_UNIT="1"), dict(PNGLOSS_HIP_SEG_UNIT="0", PNGLOSS_HIP_SEG_SEEDS1="1"), dict(PNGLOSS_HIP_SEG_UNIT="1", PNGLOSS_HIP_SEG_SEEDS="0"), dict()],
                         ids=["units-from-seeds", "segments-from-seeds", "units-from-every-state", "library-choice"])
def test_segment_engine_batches_from_seeds_match_the_oracle(torch_cuda, monkeypatch, hooks):
    """Round 6: the enumeration of a batch starts FROM SEEDS with a run-in (pl_seg_core.h: seg_enum_unit_body<.., SEEDS>) -- in units (large batches) or segment by segment
    (small and mid-size ones, seg_k_enum_unit<1>) -- instead of from every state.  Mixed batches pinned to each path, the round-5 path and the library's own choice:
    photographic frames, noise, transparency, gray classes, and FLAT few-coloured content (the suite's tux and dice, whose fixed points the seeds miss: those images fall
    back to the start from every state, seg_unit_from_seeds) -- every image against the CPU oracle, another strength / bleed pair with a seed set, NULL row_filters."""
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    g = U.load_npz("suite_small.npz")
    suite = U.load_npz("suite_inputs.npz")
    sets = [([P.synth_rgba(w, h, m, i) for i, (w, h, m) in enumerate([(1920, 28, 0), (1920, 28, 0), (1600, 24, 1), (1280, 30, 5), (1024, 26, 2), (900, 20, 3), (800, 22, 4), (1920, 18, 0),
                                                                      (700, 28, 0), (641, 19, 1), (1919, 21, 0), (97, 30, 0), (33, 9, 5), (1, 5, 1)])], 19, 2),
            ([np.ascontiguousarray(g["tux/in"]), np.ascontiguousarray(suite["dice"][:160]), np.ascontiguousarray(suite["lena"][:120]), P.synth_rgba(1920, 60, 0, 0),
              P.synth_rgba(1920, 40, 0, 7), np.ascontiguousarray(suite["ssr"][:100]), P.synth_rgba(1500, 50, 5, 3), P.synth_rgba(1200, 64, 0, 9)], 19, 2),
            ([P.synth_rgba(w, h, m, 3 + i) for i, (w, h, m) in enumerate([(1700, 20, 0), (1400, 24, 1), (1300, 16, 5), (1920, 22, 0), (960, 30, 2), (1100, 18, 4), (1800, 12, 0), (640, 25, 3)])], 12, 1)]
    ctx = P.HipContext()
    for imgs, s, b in sets:
        dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
        filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") if i != 2 else None for i, a in enumerate(imgs)]
        res = ctx.run([(d.data_ptr(), f.data_ptr() if f is not None else 0, a.shape[1], a.shape[0]) for d, f, a in zip(dev, filt, imgs)], s, b)
        torch.cuda.synchronize()
        for i, (a, d, f, r) in enumerate(zip(imgs, dev, filt, res)):
            assert ctx.engine_info(i)["engine"] == "segment-parallel"
            o1, f1 = U.run_port(a, s, b, filters=f is not None)
            assert r["status"] == 0 and np.array_equal(d.cpu().numpy(), o1), (hooks, i, a.shape, s, b)
            if f is not None:
                assert np.array_equal(f.cpu().numpy(), f1), (hooks, i, a.shape, s, b)
    ctx.close()


CAMPAIGN = [("seg", 5000, 100, 601), ("wg", 5000, 100, 602), ("", 5000, 100, 603), ("lead", 1500, 30, 604), ("mix", 1500, 30, 605)]


@pytest.mark.parametrize("engine,n_small,n_large,seed", CAMPAIGN, ids=[(c[0] or "auto") for c in CAMPAIGN])
def test_randomised_parity_campaign(torch_cuda, monkeypatch, engine, n_small, n_large, seed):
    """The randomised parity campaign INSIDE the suite the driver runs (until round 5 only profiles/r0x_fuzz_campaign.txt, run by hand, carried one): per pin of the row
    engine ("seg" segment-parallel, "wg" one workgroup per image with its own adaptive choice of chains, "" the library's choice, "lead" / "mix" the chain kinds of the
    workgroup engine) thousands of seeded random small cases and a hundred large ones (tests/util.py:fuzz_case: shapes around the segment and wave sizes, nine kinds of
    content, all byte-per-pixel classes, transparency, strengths 0..255, bleeds 1..32767, both row_filters modes) through the C ABI -- the host-pointer seam
    optimize_with_rows and, every tenth case, a device-resident batch of five mixed images -- against the CPU oracle (oracle/libpngloss_port.so, computed on host threads
    while the GPU works).  Bit-exact, every case; a mismatch names the case (seed, index) so that it can be replayed."""
    import concurrent.futures as cf
    torch = torch_cuda
    if engine:
        monkeypatch.setenv("PNGLOSS_HIP_ENGINE", engine)
    else:
        monkeypatch.delenv("PNGLOSS_HIP_ENGINE", raising=False)
    rng = np.random.default_rng(seed)
    cases = [U.fuzz_case(rng, False) for _ in range(n_small)] + [U.fuzz_case(rng, True) for _ in range(n_large)]
    U.port()                                                     # (load the oracle before the threads ask for it)
    ctx = P.HipContext()
    bad = []
    with cf.ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as pool:
        def oracle(item, s=None, b=None):
            img, s0, b0, filt = item
            return U._run_rows(U.port().port_optimize_with_rows, img, s0 if s is None else s, b0 if b is None else b, True if s is not None else filt)
        i = 0
        while i < len(cases):
            if i % 10 == 9 and i + 5 <= len(cases):
                items = cases[i:i + 5]
                s0, b0 = items[0][1], items[0][2]
                futs = [pool.submit(oracle, it, s0, b0) for it in items]
                dev = [torch.from_numpy(it[0].copy()).cuda() for it in items]
                flt = [torch.zeros(it[0].shape[0], dtype=torch.uint8, device="cuda") for it in items]
                res = ctx.run([(d.data_ptr(), f.data_ptr(), it[0].shape[1], it[0].shape[0]) for d, f, it in zip(dev, flt, items)], s0, b0)
                torch.cuda.synchronize()
                for k, (d, f, fu) in enumerate(zip(dev, flt, futs)):
                    o1, f1 = fu.result()
                    if res[k]["status"] != 0 or not (np.array_equal(o1, d.cpu().numpy()) and np.array_equal(f1, f.cpu().numpy())):
                        bad.append(("batch", seed, i + k, items[k][0].shape, s0, b0))
                i += 5
                continue
            # a window of single images: the oracle of the whole window on the host threads while the device works through it
            j = i
            while j < len(cases) and j - i < 16 and not (j % 10 == 9 and j + 5 <= len(cases)):
                j += 1
            win = cases[i:max(j, i + 1)]
            futs = [pool.submit(oracle, it) for it in win]
            for k, (it, fu) in enumerate(zip(win, futs)):
                img, s0, b0, filt = it
                o2, f2 = P.optimize_with_rows(img, s0, b0, want_filters=filt)
                o1, f1 = fu.result()
                if not (np.array_equal(o1, o2) and (not filt or np.array_equal(f1, f2))):
                    bad.append(("single", seed, i + k, img.shape, s0, b0, filt))
            i += len(win)
    ctx.close()
    assert not bad, bad[:10]


@pytest.mark.parametrize("pin,seed", [(dict(PNGLOSS_HIP_SEG_UNIT="0", PNGLOSS_HIP_SEG_SEEDS1="1"), 611), (dict(PNGLOSS_HIP_SEG_UNIT="1"), 612)], ids=["segments-from-seeds", "units-from-seeds"])
def test_randomised_parity_campaign_on_the_seeds_paths(torch_cuda, monkeypatch, pin, seed):
    """The campaign's random cases through the enumeration FROM SEEDS (round 6), which the library itself only picks for batches of wide images: pinned here for every case --
    single images and device batches of five mixed ones; strengths whose state set has no seed set run their usual path -- 3000 small and 60 large cases per pin against the
    CPU oracle.  (Random content is what the seeds like least: noise, stripes, constant and saturated images are full of cycles they miss; the rows break, finish from every
    state, images fall back -- and every byte must still be the reference's.)"""
    import concurrent.futures as cf
    torch = torch_cuda
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    for k, v in pin.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(seed)
    cases = [U.fuzz_case(rng, False) for _ in range(3000)] + [U.fuzz_case(rng, True) for _ in range(60)]
    U.port()
    ctx = P.HipContext()
    bad = []
    with cf.ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as pool:
        i = 0
        while i < len(cases):
            nb = 5 if i % 4 == 3 else 1
            items = cases[i:i + nb]
            s0, b0 = items[0][1], items[0][2]
            futs = [pool.submit(U._run_rows, U.port().port_optimize_with_rows, it[0], s0, b0, True) for it in items]
            dev = [torch.from_numpy(it[0].copy()).cuda() for it in items]
            flt = [torch.zeros(it[0].shape[0], dtype=torch.uint8, device="cuda") for it in items]
            res = ctx.run([(d.data_ptr(), f.data_ptr(), it[0].shape[1], it[0].shape[0]) for d, f, it in zip(dev, flt, items)], s0, b0)
            torch.cuda.synchronize()
            for k, (d, f, fu) in enumerate(zip(dev, flt, futs)):
                o1, f1 = fu.result()
                if res[k]["status"] != 0 or not (np.array_equal(o1, d.cpu().numpy()) and np.array_equal(f1, f.cpu().numpy())):
                    bad.append((seed, i + k, items[k][0].shape, s0, b0))
            i += len(items)
    ctx.close()
    assert not bad, bad[:10]


def _configs3_frames(indices):
    return [P.synth_rgba(1920, 1080, 0, i) for i in indices]


def test_configs3_all_256_frames_in_one_batch_match_reference_digests(torch_cuda):
    """BASELINE.json configs[3] as the TEST SUITE exercises it: all 256 frames of 1920x1080 (generator mode 0, frame = 0..255) in ONE device-resident
    batch at s=19 b=2, the library's own choice of engine; every status 0, and pixels + filter IDs of EVERY frame equal to the digests the real reference
    gave for it (tests/golden/digests_1080p.json: all 256 since round 6; digests.json: frames 0, 1, 255 as the survey measured them)."""
    torch = torch_cuda
    want = U.load_digests_1080p()
    assert sorted(want) == list(range(256))
    dev, filt = [], []
    for i in range(256):
        dev.append(torch.from_numpy(P.synth_rgba(1920, 1080, 0, i)).cuda())
        filt.append(torch.zeros(1080, dtype=torch.uint8, device="cuda"))
    ctx = P.HipContext()
    res = ctx.run([(d.data_ptr(), f.data_ptr(), 1920, 1080) for d, f in zip(dev, filt)], 19, 2)
    torch.cuda.synchronize()
    assert len(res) == 256 and all(r["status"] == 0 and r["bpp"] == 4 for r in res)
    for i, e in sorted(want.items()):
        assert "%016x" % P.fnv1a64(dev[i].cpu().numpy(), P.SURVEY_FNV_BASIS) == e["out"], i
        assert "%016x" % P.fnv1a64(filt[i].cpu().numpy(), P.SURVEY_FNV_BASIS) == e["filters"], i
    ctx.close()


@pytest.mark.parametrize("share", [32, 64])
def test_configs3_rank_shares_match_reference_digests(torch_cuda, share):
    """What ONE rank of an N = 8 / N = 4 node gets of configs[3] (shard.contiguous_partition: 32 / 64 consecutive frames), run here as the LAST rank's
    share and as the FIRST rank's; every frame is checked against its reference digest."""
    torch = torch_cuda
    from pngloss_amd import shard as S
    want = U.load_digests_1080p()
    parts = S.contiguous_partition(256, 256 // share)
    ctx = P.HipContext()
    for mine in (parts[-1], parts[0]):
        dev = [torch.from_numpy(P.synth_rgba(1920, 1080, 0, i)).cuda() for i in mine]
        filt = [torch.zeros(1080, dtype=torch.uint8, device="cuda") for _ in mine]
        res = ctx.run([(d.data_ptr(), f.data_ptr(), 1920, 1080) for d, f in zip(dev, filt)], 19, 2)
        torch.cuda.synchronize()
        assert all(r["status"] == 0 for r in res)
        known = [i for i in mine if i in want]
        assert len(known) == len(mine)
        for i in known:
            k = i - mine[0]
            assert "%016x" % P.fnv1a64(dev[k].cpu().numpy(), P.SURVEY_FNV_BASIS) == want[i]["out"], i
            assert "%016x" % P.fnv1a64(filt[k].cpu().numpy(), P.SURVEY_FNV_BASIS) == want[i]["filters"], i
    ctx.close()


def test_configs3_on_eight_contexts_of_one_device_like_a_node_of_eight():
    """Multi-GPU readiness a one-GPU box can prove: pngloss_hip_multi with devices "0,0,0,0,0,0,0,0" -- EIGHT contexts, eight host threads, eight launch
    threads on the one device -- takes configs[3]'s 256 frames from host memory, deals them out (32 each: equal sizes), and every one of the 256 frames
    comes back equal to its reference digest.  (On a node the same call opens one context per GPU; nothing else differs.)"""
    want = U.load_digests_1080p()
    imgs = _configs3_frames(range(256))
    assert sorted(np.bincount(P.multi_split([(1920, 1080)] * 256, 8)).tolist()) == [32] * 8
    multi = P.HipMulti("0,0,0,0,0,0,0,0")
    assert multi.count == 8
    outs, filts, res = multi.run_host(imgs, 19, 2)
    multi.close()
    assert all(r["status"] == 0 for r in res)
    for i, e in sorted(want.items()):
        assert "%016x" % P.fnv1a64(outs[i], P.SURVEY_FNV_BASIS) == e["out"], i
        assert "%016x" % P.fnv1a64(filts[i], P.SURVEY_FNV_BASIS) == e["filters"], i

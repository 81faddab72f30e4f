"""GPU tests of the quantiser's colour-count search (include/pngloss_hip_quant_target.h): pngloss_hip_quantize_batch_target and its multi host form
against the procedure restated over tests/util_quant.py and tests/util_dither.py -- the chosen N, the probes and their verdicts, the pixels and the
whole report, by equality --, against pngloss_hip_quantize_batch2 at the chosen N on a fresh copy, a batch whose images probe different N in one
round against its images alone, the device loops of pl_quant_measure past one trip, dithering, and the tool's --colors M --colors-psnr DB."""
import math
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D
from tests import util_index as X
from tests import util_quant as Q
from tests import util_quant_target as T

pytestmark = pytest.mark.gpu

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
FS = P.lib.DITHER_FLOYD_STEINBERG
INF = math.inf


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def images():
    inputs = U.load_npz("suite_inputs.npz")
    shapes = Q.shapes()
    return dict(rose=inputs["rose"], tux=inputs["tux"], checker_64x48=shapes["checker_64x48"][0], flat_64x16=shapes["flat_64x16"][0],
                one=shapes["1x1"][0], empty=np.zeros((0, 0, 4), np.uint8))


PROBES = {}


def _probes(images, name, rounds=8, dither=0):
    """the restated probes of an image: each N restated once for the whole module"""
    key = (name, rounds, dither)
    if key not in PROBES:
        PROBES[key] = T.Probes(images[name], rounds, dither)
    return PROBES[key]


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


def _target_run(ctx, arrays, m, psnr=0.0, max_abs=0, rounds=8, dither=0):
    dev, descs = _upload(arrays)
    _, reports = ctx.quantize_target(descs, P.lib.QuantTarget(psnr, max_abs), m, rounds, dither)
    return _download(dev, arrays), reports


def _plain_run(ctx, arrays, n, rounds=8, dither=0):
    dev, descs = _upload(arrays)
    _, reports = ctx.quantize(descs, n, rounds, dither=dither)
    return _download(dev, arrays), reports


def _check(ctx, name, img, out, rep, want, rounds=8, dither=0):
    """one image's answer against the restated procedure, and against pngloss_hip_quantize_batch2 at the chosen N on a fresh copy"""
    T.same_report(name, rep, want)
    assert np.array_equal(out, want["quant"]["pixels"]), name
    plain_out, plain_rep = _plain_run(ctx, [img], rep["colors"], rounds, dither)
    assert np.array_equal(out, plain_out[0]) and rep["quant"] == plain_rep[0], name
    assert rep["quant"]["distortion"] == D.np_distortion(img, out), name
    if not dither:
        assert rep["probe_distortion"] == rep["quant"]["distortion"], name


CASES = {
    # name: (image, M, min_psnr_db, max_abs_error)
    "rose_30dB": ("rose", 256, 30.0, 0),
    "rose_max_error_60": ("rose", 256, 0.0, 60),
    "rose_both": ("rose", 256, 30.0, 60),
    "tux_38dB": ("tux", 256, 38.0, 0),
    "tux_only_exact": ("tux", 256, INF, 0),
    "rose_16_not_reached": ("rose", 16, 38.0, 0),
    "rose_M_2": ("rose", 2, 30.0, 0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_single_image_against_the_restated_procedure(ctx, images, case):
    name, m, psnr, max_abs = CASES[case]
    img = images[name]
    p = _probes(images, name)
    want = p.search(m, psnr, max_abs)
    print(case, want["colors"], want["probed"], bin(want["accepted_mask"]), "margin %.2e dB" % p.margin(want, psnr))
    assert not psnr or p.margin(want, psnr) >= 1e-6                  # C's and Python's log10 cannot disagree on a probe
    outs, reports = _target_run(ctx, [img], m, psnr, max_abs)
    _check(ctx, case, img, outs[0], reports[0], want)
    rep = reports[0]
    if case == "rose_30dB":
        assert (rep["colors"], rep["probes"], rep["reached"]) == (27, 9, 1)
    elif case == "rose_both":                                        # the two conditions together ask for more than either alone
        alone = (p.search(m, psnr, 0)["colors"], p.search(m, 0.0, max_abs)["colors"])
        assert rep["colors"] >= max(alone) and max(rep["quant"]["distortion"]["max_abs"]) <= 60
    elif case == "rose_max_error_60":
        assert max(rep["quant"]["distortion"]["max_abs"]) <= 60 and rep["reached"] == 1
    elif case == "tux_38dB":
        assert (rep["colors"], rep["reached"]) == (20, 1)
    elif case == "tux_only_exact":
        assert (rep["colors"], rep["reached"], rep["quant"]["colors_in"], rep["quant"]["exact"]) == (194, 1, 194, 1) and np.array_equal(outs[0], img)
        assert rep["probed"] == [256, 128, 192, 224, 208, 200, 196, 194, 193] and rep["quant"]["distortion"]["changed_pixels"] == 0
    elif case == "rose_16_not_reached":
        assert (rep["colors"], rep["reached"], rep["probes"], rep["accepted_mask"], rep["probed"]) == (16, 0, 1, 0, [16])
    elif case == "rose_M_2":
        assert (rep["colors"], rep["probes"], rep["probed"]) == (2, 1, [2])


def test_an_image_without_pixels_and_a_1x1_image_in_the_batch(ctx, images):
    names = ["empty", "rose", "one", "empty"]
    arrays = [images[k] for k in names]
    outs, reports = _target_run(ctx, arrays, 256, 30.0)
    for k, img, out, rep in zip(names, arrays, outs, reports):
        want = _probes(images, k).search(256, 30.0)
        T.same_report(k, rep, want)
        assert np.array_equal(out, want["quant"]["pixels"]), k
        if k != "rose":                                              # every probe is exact: none of them ran on the device
            assert (rep["colors"], rep["reached"], rep["probes"], rep["accepted_mask"], rep["quant"]["exact"]) == (2, 1, 8, 0xFF, 1), k
            assert rep["probed"] == [256, 128, 64, 32, 16, 8, 4, 2], k
            assert rep["probe_distortion"]["pixels"] == img.size // 4 and rep["probe_distortion"]["changed_pixels"] == 0
    assert reports[0]["quant"]["colors_in"] == 0 and reports[2]["quant"]["colors_in"] == 1


MIXED = ["rose", "tux", "checker_64x48", "flat_64x16"]


@pytest.fixture(scope="module")
def mixed(ctx, images):
    arrays = [images[k] for k in MIXED]
    return arrays, _target_run(ctx, arrays, 256, 30.0)


def test_images_that_probe_different_counts_in_one_round(ctx, images, mixed):
    arrays, (outs, reports) = mixed
    for k, img, out, rep in zip(MIXED, arrays, outs, reports):
        want = _probes(images, k).search(256, 30.0)
        _check(ctx, k, img, out, rep, want)
        one_out, one_rep = _target_run(ctx, [img], 256, 30.0)
        assert np.array_equal(out, one_out[0]) and rep == one_rep[0], k
    probed = [r["probed"] for r in reports]
    assert len({p[4] for p in probed[:3]}) == 2 and len({p[5] for p in probed[:3]}) == 3    # one round, three colour counts: one job table, a different `entries` per job
    assert reports[3]["quant"]["exact"] == 1 and reports[3]["colors"] == 2 and reports[2]["quant"]["colors_in"] > 4


def test_multi_host_form_equals_the_device_form(images, mixed):
    arrays, (outs, reports) = mixed
    arrays = arrays + [images["empty"], images["one"]]
    assert set(P.multi_split([(a.shape[1], a.shape[0]) for a in arrays], 2)) == {0, 1}
    m = P.HipMulti("0,0")
    try:
        host_outs, host_reports = m.quantize_host_target(arrays, P.lib.QuantTarget(30.0), 256, 8)
        for bad in (P.lib.QuantTarget(0.0, 0), P.lib.QuantTarget(-1.0), P.lib.QuantTarget(30.0, 256)):
            with pytest.raises(RuntimeError):
                m.quantize_host_target(arrays, bad, 256, 8)
    finally:
        m.close()
    for k, a, b, ra, rb in zip(MIXED, outs, host_outs, reports, host_reports):
        assert np.array_equal(a, b) and ra == rb, k
    assert host_reports[4]["quant"]["colors_in"] == 0 and host_reports[5]["quant"]["exact"] == 1 and np.array_equal(host_outs[5], images["one"])


def test_refusals_on_a_live_context_write_nothing(ctx, images):
    img = images["rose"]
    dev, descs = _upload([img])
    for target, m, rounds, dither in ((P.lib.QuantTarget(0.0, 0), 256, 8, 0), (P.lib.QuantTarget(math.nan), 256, 8, 0), (P.lib.QuantTarget(30.0, 256), 256, 8, 0),
                                      (P.lib.QuantTarget(30.0, 0, 1), 256, 8, 0), (P.lib.QuantTarget(30.0), 1, 8, 0), (P.lib.QuantTarget(30.0), 256, 65, 0),
                                      (P.lib.QuantTarget(30.0), 256, 8, 2)):
        with pytest.raises(RuntimeError):
            ctx.quantize_target(descs, target, m, rounds, dither)
    with pytest.raises(RuntimeError):
        ctx.quantize_target([(0, 0, 4, 4)], P.lib.QuantTarget(30.0))                    # pixels, and no pointer
    assert np.array_equal(_download(dev, [img])[0], img)


# ---- the device loops past one trip ----

def test_a_workgroup_of_the_measuring_pass_takes_a_second_chunk_in_a_batch(ctx):
    """256 working images get 8 workgroups each, sized by the 10 chunks of the large image in the middle: two of its workgroups take two chunks.
    M = 2: one probe, and the result is the N = 2 call's"""
    batch, n, rounds = Q.device_shapes()["two_chunks_in_a_batch"]
    assert n == 2 and len(batch) == 256 and Q.want_blocks(256) == 8 and Q.busiest_wg_pixels(100 * 100, 256) >= 2 * Q.CHUNK
    outs, reports = _target_run(ctx, batch, 2, 20.0, 0, rounds)
    plain_outs, plain_reports = _plain_run(ctx, batch, 2, rounds)
    for i, (img, out, rep) in enumerate(zip(batch, outs, reports)):
        want = Q.restate(img, 2, rounds)
        assert (rep["colors"], rep["probes"], rep["probed"]) == (2, 1, [2]) and rep["reached"] == int(T.accepts(want["distortion"], 20.0)), i
        assert np.array_equal(out, want["pixels"]) and np.array_equal(out, plain_outs[i]) and rep["quant"] == plain_reports[i], i
        assert rep["probe_distortion"] == rep["quant"]["distortion"] == want["distortion"], i
    assert {r["reached"] for r in reports} == {0, 1}


def _torch_record(a, b):
    """the record of two device tensors of RGBA8 bytes (b against a), from torch's integer sums"""
    import torch
    d = b.view(-1, 4).to(torch.int64) - a.view(-1, 4).to(torch.int64)
    changed = int((a.view(torch.int32) != b.view(torch.int32)).sum().item())
    return dict(pixels=a.numel() // 4, changed_pixels=changed, sq_err=[int(v) for v in (d * d).sum(dim=0).tolist()], max_abs=[int(v) for v in d.abs().amax(dim=0).tolist()])


def _noise_image(pixels, seed, colours=4096):
    """`pixels` words drawn on the device from `colours` random RGBA8 words, as bytes: at two colours every channel is far from its entry"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    pool = torch.randint(-(1 << 31), 1 << 31, (colours,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    return pool[torch.randint(0, colours, (pixels,), generator=g, device="cuda")].view(torch.uint8)


def test_channel_sums_past_32_bits_in_one_probe(ctx):
    """the size of the sums_past_32_bits recipe, 4608x4096, at M = 2, one probe.  The recipe's three words would leave squared errors of 3e7 a
    channel -- it is the assign pass's sums of pixel VALUES that they take past 2^32 --, so the pixels here are noise: the record's squared-error
    sums are past 2^32, which only 64-bit merging carries.  (Alone, the image gets 1024 workgroups: a lane takes 72 pixels.  The next test takes a
    lane past its flush.)"""
    import torch
    w, h, rounds = 4608, 4096, 2
    img = _noise_image(w * h, 61)
    work = img.clone()
    torch.cuda.synchronize()
    _, reports = ctx.quantize_target([(work.data_ptr(), 0, w, h)], P.lib.QuantTarget(20.0), 2, rounds)
    fresh = img.clone()
    _, plain = ctx.quantize([(fresh.data_ptr(), 0, w, h)], 2, rounds, dither=0)
    torch.cuda.synchronize()
    rep = reports[0]
    rec = _torch_record(img, work)
    print("sums_past_32_bits", rec)
    assert min(rec["sq_err"]) > 1 << 32 and Q.blocks(w * h, Q.want_blocks(1)) == Q.MAX_BLOCKS == 1024
    assert (rep["colors"], rep["probes"], rep["probed"]) == (2, 1, [2]) and rep["reached"] == int(T.accepts(rec, 20.0))
    assert torch.equal(work, fresh) and rep["quant"] == plain[0]
    assert rep["probe_distortion"] == rep["quant"]["distortion"] == rec


def test_a_lane_of_the_measuring_pass_is_taken_past_its_flush(ctx):
    """in a batch of 256 working images an image gets 8 workgroups however large it is: one of 5800x5800 pixels gives every lane more than the
    PLD_FLUSH_PIXELS = 16384 pixels after which it empties its 32-bit sums into the 64-bit ones.  (What the sums would do without the flush, past
    66 051 pixels a lane, is the CPU harness's to show: on the device that takes an image of half a gigabyte.)"""
    import torch
    side, rounds = 5800, 1
    assert Q.want_blocks(256) == 8 and Q.busiest_wg_pixels(side * side, 256) // 256 > 16384 + 4
    small, n, _ = Q.device_shapes()["two_chunks_in_a_batch"]
    small = [a for a in small if a.shape[0] == 2][:255]
    big = _noise_image(side * side, 67)
    work = big.clone()
    dev, descs = _upload(small)
    descs.insert(100, (work.data_ptr(), 0, side, side))
    _, reports = ctx.quantize_target(descs, P.lib.QuantTarget(20.0), 2, rounds)
    outs = _download(dev, small)
    fresh = big.clone()
    dev2, descs2 = _upload(small)
    descs2.insert(100, (fresh.data_ptr(), 0, side, side))
    _, plain = ctx.quantize(descs2, 2, rounds, dither=0)
    plain_outs = _download(dev2, small)
    rep = reports.pop(100)
    plain_big = plain.pop(100)
    rec = _torch_record(big, work)
    assert torch.equal(work, fresh) and rep["quant"] == plain_big and rep["probe_distortion"] == rep["quant"]["distortion"] == rec
    assert (rep["colors"], rep["probes"]) == (2, 1) and rec["changed_pixels"] > 0
    for i, (a, out, r) in enumerate(zip(small, outs, reports)):
        assert np.array_equal(out, plain_outs[i]) and r["quant"] == plain[i] and r["probe_distortion"] == r["quant"]["distortion"] == D.np_distortion(a, out), i


# ---- dithering ----

def test_dithered_search_equals_the_procedure_over_the_dithered_restatement(ctx, images):
    img = images["rose"]
    p = _probes(images, "rose", 8, 1)
    want = p.search(256, 30.0)
    assert p.margin(want, 30.0) >= 1e-6
    outs, reports = _target_run(ctx, [img], 256, 30.0, 0, 8, FS)
    _check(ctx, "rose_dithered", img, outs[0], reports[0], want, 8, FS)
    plain = _probes(images, "rose").search(256, 30.0)
    print("rose at 30 dB: dithered", want["colors"], want["probed"], "nearest entry", plain["colors"], plain["probed"])
    assert reports[0]["reached"] == 1 and not np.array_equal(outs[0], plain["quant"]["pixels"])
    # that search ends on an earlier probe than its last, so the close ran the pass again for the palette it kept; at 35 dB the last probe is the
    # chosen one and its result lies there already
    assert want["probed"][-1] != want["colors"]
    there = p.search(256, 35.0)
    assert there["probed"][-1] == there["colors"] and p.margin(there, 35.0) >= 1e-6
    outs, reports = _target_run(ctx, [img], 256, 35.0, 0, 8, FS)
    _check(ctx, "rose_dithered_35dB", img, outs[0], reports[0], there, 8, FS)


# ---- the tool ----

@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")
def test_tool_chooses_the_colour_count(images, tmp_path):
    from PIL import Image
    img = images["rose"]
    want = _probes(images, "rose").search(256, 30.0)                  # (the tool's rounds: PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS)
    src, out = str(tmp_path / "rose.png"), str(tmp_path / "rose-30dB.png")
    Image.fromarray(img, "RGBA").save(src)
    r = subprocess.run([OUR_CLI, "-f", "--colors", "256", "--colors-psnr", "30", "--distortion", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    im = Image.open(out)
    assert im.mode == "P"
    pixels = np.asarray(im.convert("RGBA"))
    assert np.array_equal(pixels, want["quant"]["pixels"]) and len(np.unique(Q.words(pixels))) == want["quant"]["entries"] <= want["colors"]
    ch = dict(X.chunks_of(open(out, "rb").read()))
    assert ch[b"IHDR"][8:10] == b"\x08\x03" and len(ch[b"PLTE"]) == 3 * want["quant"]["entries"]
    lines = r.stderr.splitlines()
    at = lines.index("  colors: more than 256 in the input, %d palette entries" % want["quant"]["entries"])
    assert lines[at + 1] == "  chosen: %d of at most 256 colours, %.2f dB (%d probes)" % (want["colors"], D.py_psnr_db(want["quant"]["distortion"], 0xF), want["probes"])
    assert D.cli_line(want["quant"]["distortion"], 3) in lines, r.stderr       # (rose is opaque colour: three stored channels)
    assert "colour target" not in r.stderr
    # a target that 4 colours do not reach: the file is written at 4 colours, with a warning
    r = subprocess.run([OUR_CLI, "-f", "--colors", "4", "--colors-psnr", "30", "-v", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "  chosen: 4 of at most 4 colours, target not reached" in r.stderr.splitlines()
    assert any(line.startswith("  warning: ") and "written at 4 colours" in line for line in r.stderr.splitlines()), r.stderr
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), Q.restate(img, 4, 8)["pixels"])
    r = subprocess.run([OUR_CLI, "-f", "--colors-psnr", "30", "-o", out, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == P.lib.PNGLOSS_INVALID_ARGUMENT and r.stderr == "--colors-psnr requires --colors.\n"

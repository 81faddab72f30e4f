"""GPU tests of pngloss_hip_optimize_batch_target and its host form: the strength the library finds for an image is the one the rule gives on the CPU
oracle, and the image then holds what a plain batch at that strength writes.

Every expectation comes from the CPU oracle (U.run_port), numpy (tests/util_distort.py) and the rule restated in Python (tests/util_target.py);
tests/test_target_oracle.py pins what those give for the fixed cases, so each branch of the search is known to run here.  Equality is exact."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_distort as D
from tests import util_target as T

pytestmark = pytest.mark.gpu

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
#: the one call that carries every fixed case, an image without pixels and a 48 x 12 mode-5 image: a call has ONE target, so the mixed batch runs under
#: the two targets of the fixed cases -- its searches part ways round by round (tests/test_target_oracle.py counts the strengths per round)
MIXED = [c[0] for c in T.CASES] + [(0, 0, 0), (48, 12, 5)]
#: Under 51.6 dB with M = 3 the mixed batch ends on the two closing paths that share the last move table: three images accept strength 1 and are refused at 2
#: afterwards (the stash goes back), the other three accept nothing (the original goes back and strength 0 runs once) -- on the oracle strength 1 gives
#: 51.84 / 51.12 / 51.72 / 52.47 / 50.97 / 51.41 dB in the order of MIXED.  Under the two targets above an image ends either in place or from the stash.
SETUPS = [("case%d" % k, [c[0]], (c[2], c[3], c[1])) for k, c in enumerate(T.CASES)] + [("mixed_35dB_M19", MIXED, (35.0, 0, 19)), ("mixed_39dB_err8_M40", MIXED, (39.0, 8, 40)),
                                                                                     ("mixed_51.6dB_M3", MIXED, (51.6, 0, 3))]
REFERENCE_FIELDS = ("status", "bpp", "unique_symbols", "retried_rows")


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C").reshape(-1)).cuda()


def _device_batch(imgs):
    import torch
    dev = [_dev(a) for a in imgs]
    flt = [torch.zeros(max(a.shape[0], 1), dtype=torch.uint8, device="cuda") for a in imgs]
    desc = [(d.data_ptr() if a.size else 0, f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)]
    return dev, flt, desc


def _back(dev, flt, imgs):
    import torch
    torch.cuda.synchronize()
    return [d.cpu().numpy().reshape(a.shape) for d, a in zip(dev, imgs)], [f.cpu().numpy()[: a.shape[0]] for f, a in zip(flt, imgs)]


def _expected(shape, target):
    psnr, max_abs, m = target
    chosen, seq, _ = T.oracle_search(shape, m, psnr, max_abs)
    accepted_any = chosen > 0 or (chosen == m)
    runs = len(seq) + (0 if accepted_any else 1)                 # nothing accepted below M > 0: strength 0 is run once at the end
    return chosen, seq, runs


def _check_call(ctx, shapes, target, stream=0):
    """one target call on fresh copies of the shapes' images; everything the contract promises is compared.  Returns the reports."""
    imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
    dev, flt, desc = _device_batch(imgs)
    res, rep = ctx.run_target(desc, P.Target(*target), T.BLEED, stream=stream)
    outs, filts = _back(dev, flt, imgs)
    for i, (shape, img) in enumerate(zip(shapes, imgs)):
        chosen, seq, runs = _expected(shape, target)
        assert (rep[i].strength, rep[i].probes, rep[i].runs) == (chosen, len(seq), runs), (shape, target, rep[i].as_dict(), seq)
        assert rep[i].probes <= T.py_probe_bound(target[2])
        _, want, want_f, want_rec, want_bpp = T.oracle_probe(*shape, chosen)
        assert np.array_equal(outs[i], want) and np.array_equal(filts[i], want_f), (shape, target)
        assert rep[i].distortion.as_dict() == want_rec == D.np_distortion(img, outs[i]), shape
        if not img.size:
            continue
        # a plain batch at that strength on a fresh copy: the same bytes, the same record
        pdev, pflt, pdesc = _device_batch([img])
        plain = ctx.run(pdesc, chosen, T.BLEED)
        pouts, pfilts = _back(pdev, pflt, [img])
        assert np.array_equal(outs[i], pouts[0]) and np.array_equal(filts[i], pfilts[0]), shape
        # (repaired_pixels, the fifth slot, is a diagnostic of the run that produced it: the engine's own bookkeeping, not part of the result)
        assert {k: res[i][k] for k in REFERENCE_FIELDS} == {k: plain[0][k] for k in REFERENCE_FIELDS}, (shape, res[i], plain[0])
        assert res[i]["status"] == 0 and res[i]["bpp"] == want_bpp
    return rep


@pytest.mark.parametrize("engine", ["auto", "seg", "wg"])
@pytest.mark.parametrize("setup", SETUPS, ids=[s[0] for s in SETUPS])
def test_chosen_strength_and_bytes_equal_the_oracle_rule(setup, engine):
    _, shapes, target = setup
    ctx = P.HipContext()
    try:
        ctx.set_option("engine", engine)
        rep = _check_call(ctx, shapes, target)
    finally:
        ctx.close()
    if len(shapes) > 1:
        assert len({r.strength for r in rep}) >= 3               # the searches of one call ended in different places
        assert rep[MIXED.index((0, 0, 0))].as_dict() == dict(strength=target[2], probes=1, runs=1, distortion=dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4))


def test_stream_of_the_callers_option_distortion_and_the_context_afterwards():
    import torch
    lib = P.hip_lib()
    shapes, target = MIXED, (35.0, 0, 19)
    ctx = P.HipContext()
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        first = [r.as_dict() for r in _check_call(ctx, shapes, target, stream=st.cuda_stream)]
        # right after the call no single batch exists to index
        out, hist, info = P.Distortion(), np.zeros(256, np.uint32), (L.C.c_int32 * 8)()

        def queries():
            return (lib.pngloss_hip_last_distortion(ctx._ctx, 0, out), lib.pngloss_hip_last_histogram(ctx._ctx, 0, hist.ctypes.data_as(L.C.c_void_p)),
                    lib.pngloss_hip_last_engine_info(ctx._ctx, 0, info))

        imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
        dev, flt, desc = _device_batch(imgs)
        ctx.run_target(desc, P.Target(*target), T.BLEED)
        assert queries() == (L.PNGLOSS_INVALID_ARGUMENT,) * 3
        # the option "distortion" plays no part and is left as the caller set it: on, the same reports, and the next plain batch is measured
        ctx.set_option("distortion", "on")
        assert [r.as_dict() for r in _check_call(ctx, shapes, target)] == first
        dev, flt, desc = _device_batch(imgs)
        ctx.run_target(desc, P.Target(*target), T.BLEED)
        assert queries() == (L.PNGLOSS_INVALID_ARGUMENT,) * 3
        w, h, mode = shapes[0]
        img, want, want_f, want_rec, _ = T.oracle_probe(w, h, mode, 19)
        pdev, pflt, pdesc = _device_batch([img])
        assert ctx.run(pdesc, 19, T.BLEED)[0]["status"] == 0
        pouts, pfilts = _back(pdev, pflt, [img])
        assert np.array_equal(pouts[0], want) and np.array_equal(pfilts[0], want_f) and ctx.distortion(0).as_dict() == want_rec
        # ... and off again: the same reports, the next plain batch equals the oracle and is not measured
        ctx.set_option("distortion", "off")
        assert [r.as_dict() for r in _check_call(ctx, shapes, target)] == first
        pdev, pflt, pdesc = _device_batch([img])
        ctx.run(pdesc, 19, T.BLEED)
        pouts, pfilts = _back(pdev, pflt, [img])
        assert np.array_equal(pouts[0], want) and np.array_equal(pfilts[0], want_f)
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_last_histogram(ctx._ctx, 0, hist.ctypes.data_as(L.C.c_void_p)) == 0
        # images without row filters, and a call without images
        dev, _, desc = _device_batch(imgs[:2])
        res, rep = ctx.run_target([(p, 0, w_, h_) for (p, _, w_, h_) in desc], P.Target(*target), T.BLEED)
        outs, _ = _back(dev, [torch.zeros(1, dtype=torch.uint8, device="cuda")] * 2, imgs[:2])
        for k in range(2):
            want_null = U.run_port(imgs[k], rep[k].strength, T.BLEED, filters=False)[0]
            assert np.array_equal(outs[k], want_null), k
        assert ctx.run_target([], P.Target(*target), T.BLEED) == ([], [])
    finally:
        ctx.close()


@pytest.mark.parametrize("emit", ["scanlines", "zlib"])
def test_host_images_on_two_contexts(emit):
    shapes, target = MIXED, (35.0, 0, 19)
    imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
    multi = P.HipMulti("0,0")
    ctx = P.HipContext()
    try:
        assert multi.count == 2
        outs, filts, res, rep, emitted = multi.run_host_target(imgs, P.Target(*target), T.BLEED, emit=emit)
        with pytest.raises(RuntimeError):
            multi.distortion(0)
        for i, (shape, img) in enumerate(zip(shapes, imgs)):
            chosen, seq, _ = _expected(shape, target)
            assert (rep[i].strength, rep[i].probes) == (chosen, len(seq)) and rep[i].probes <= rep[i].runs <= rep[i].probes + 1, (shape, rep[i].as_dict())
            _, want, want_f, want_rec, want_bpp = T.oracle_probe(*shape, chosen)
            assert np.array_equal(outs[i], want) and np.array_equal(filts[i], want_f), shape
            assert rep[i].distortion.as_dict() == want_rec, shape
            if not img.size:
                continue
            assert res[i]["status"] == 0 and res[i]["bpp"] == want_bpp
            # the host path at the chosen strength, this image alone: the same outputs
            pouts, pfilts, plain = ctx.run_host_emit([img], chosen, T.BLEED)
            assert np.array_equal(pouts[0], outs[i]) and np.array_equal(pfilts[0], filts[i])
            ctype, ids, rows = plain[0]
            if emit == "scanlines":
                assert emitted[i][0] == ctype and np.array_equal(emitted[i][1], ids) and np.array_equal(emitted[i][2], rows), shape
            else:
                raw = zlib.decompress(emitted[i][1])
                assert emitted[i][0] == ctype and raw == b"".join(bytes([int(t)]) + r.tobytes() for t, r in zip(ids, rows)), shape
    finally:
        ctx.close()
        multi.close()


def _decode(data):
    from PIL import Image
    p = L.parse_png(data)
    stride = len(p["scanlines"]) // p["height"]
    filters = bytes(p["scanlines"][y * stride] for y in range(p["height"]))
    return np.array(Image.open(io.BytesIO(data)).convert("RGBA")), filters


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers on this box)")
def test_tool_writes_the_files_of_the_chosen_strengths(tmp_path):
    from PIL import Image
    shapes = [(64, 8, 0), (33, 16, 2), (130, 6, 3)]
    target = (35.0, 0, 19)
    names = ["a", "b", "c"]
    chosen = [_expected(s, target)[0] for s in shapes]
    assert len(set(chosen)) >= 2
    src = tmp_path / "src"
    src.mkdir()
    for n, (w, h, mode) in zip(names, shapes):
        Image.fromarray(T.oracle_probe(w, h, mode, 0)[0], "RGBA").save(src / f"{n}.png")

    def run(tag, args, files, ok=(0,)):
        d = tmp_path / tag
        d.mkdir()
        for n in files:
            (d / f"{n}.png").write_bytes((src / f"{n}.png").read_bytes())
        r = subprocess.run([OUR_CLI] + args + [str(d / f"{n}.png") for n in files], capture_output=True, text=True, timeout=300)
        assert r.returncode in ok, (tag, r.stderr[-800:])
        return [(d / f"{n}-loss.png").read_bytes() if r.returncode == 0 else None for n in files], r.stderr.splitlines()

    got, err = run("target", ["--target-psnr", "35", "-s", "19", "-v"], names)
    lines = [x for x in err if x.startswith("  strength ")]
    assert lines == ["  strength %d chosen in %d probes" % (_expected(s, target)[0], len(_expected(s, target)[1])) for s in shapes], err
    for n, c, data in zip(names, chosen, got):
        plain, _ = run(f"plain_{n}", ["-s", str(c)], [n])
        assert plain[0] == data, n                                # byte-identical files (zlib on the host both times)
    # the device read and deflate paths and the distortion line, which comes from the report: compared on decoded pixels and filter bytes
    got2, err2 = run("target_gpu", ["--target-psnr", "35", "-s", "19", "-v", "--gpu-read", "--gpu-deflate", "--distortion"], names)
    assert [x for x in err2 if x.startswith("  strength ")] == lines
    want_lines = []
    for n, shape, c, data in zip(names, shapes, chosen, got2):
        img, want, want_f, rec, bpp = T.oracle_probe(*shape, c)
        px, filt = _decode(data)
        plain, _ = run(f"plain_gpu_{n}", ["-s", str(c), "--gpu-read", "--gpu-deflate"], [n])
        ppx, pfilt = _decode(plain[0])
        assert np.array_equal(px, want) and np.array_equal(px, ppx) and filt == pfilt, n
        want_lines.append(D.cli_line(rec, bpp))
    assert [x for x in err2 if x.startswith("  distortion:")] == want_lines
    # --max-error goes through the same call, and so does --skip-if-larger (98: the tiny result was not smaller than its input, nothing is written)
    c3, seq3, _ = _expected(shapes[0], (0.0, 8, 40))
    got3, err3 = run("maxerr", ["--max-error", "8", "-s", "40", "-v"], ["a"])
    assert "  strength %d chosen in %d probes" % (c3, len(seq3)) in err3
    assert np.array_equal(_decode(got3[0])[0], T.oracle_probe(*shapes[0], c3)[1])
    _, err4 = run("skip", ["--max-error", "8", "-s", "40", "-v", "--skip-if-larger"], ["a"], ok=(0, 98))
    assert "  strength %d chosen in %d probes" % (c3, len(seq3)) in err4

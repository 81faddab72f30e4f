"""GPU tests of the SSIM measurement: pngloss_hip_compare_batch_ssim on every shape and content of tests/util_ssim.py, in a call of 260 pairs
(8 workgroups per image: tile after tile over one LDS table, sums past 32 bits) and in one of 65 540 (a second launch), the option "ssim" on every
optimise entry point (outputs unchanged, records equal to the definition on original and oracle output), pngloss_hip_optimize_batch_target2
against the committed table of the CPU oracle (tests/golden/ssim_target_table.json), the multi-device wrapper and the two command line switches.

Every expected record comes from the definition restated in Python integers (tests/util_ssim.py:py_ssim), the optimised pixels from the CPU oracle
(U.run_port); equality is exact.  The mean only appears in the tool's text, formatted by the same formula in Python."""
import io
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_distort as D
from tests import util_ssim as S
from tests import util_target as T
from tests import util_visible as V

pytestmark = pytest.mark.gpu

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
NO_WINDOWS = dict(windows=0, sum_q16=[0] * 4, min_q16=[65536] * 4, reserved=0)
TABLE = S.load_table()


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


# ------------------------------------------------------------------------------------------------ compare_batch_ssim

def test_compare_every_shape_and_content_in_one_mixed_call():
    cases = S.all_cases()
    dev = [(_dev(a), _dev(b)) for _, a, b in cases]
    ctx = P.HipContext()
    try:
        got = ctx.compare_ssim([(da.data_ptr() if a.size else 0, db.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for (da, db), (_, a, _) in zip(dev, cases)])
        assert ctx.compare_ssim([]) == []
    finally:
        ctx.close()
    for (name, a, b), g in zip(cases, got):
        assert g.as_dict() == S.expected(name), name
    by = {n: g.as_dict() for (n, _, _), g in zip(cases, got)}
    assert by["0x0_noise"] == by["7x64_noise"] == by["257x5_equal"] == NO_WINDOWS
    assert by["300x77_equal"]["windows"] == 74 * 18 and got[[n for n, _, _ in cases].index("300x77_equal")].mean(0xF) == 1.0


def test_compare_bases_off_16_byte_alignment():
    import torch
    picked = [c for c in S.all_cases() if c[0] in ("12x12_noise", "131x69_oracle", "300x77_noise")]
    assert len(picked) == 3
    ctx = P.HipContext()
    try:
        for name, a, b in picked:
            n = a.size
            big_a, big_b = torch.zeros(n + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
            assert big_a.data_ptr() % 16 == 0 and big_b.data_ptr() % 16 == 0
            for oa, ob in ((4, 0), (0, 8), (12, 12)):
                va, vb = big_a[oa:oa + n], big_b[ob:ob + n]
                va.copy_(torch.from_numpy(a.reshape(-1))); vb.copy_(torch.from_numpy(b.reshape(-1)))
                torch.cuda.synchronize()
                assert va.data_ptr() % 16 == oa and vb.data_ptr() % 16 == ob
                assert ctx.compare_ssim([(va.data_ptr(), vb.data_ptr(), a.shape[1], a.shape[0])])[0].as_dict() == S.expected(name), (name, oa, ob)
    finally:
        ctx.close()


def _pair_descs(cases):
    """(name, a, b) cases on the device: (the tensors, to be kept, and one (d_a, d_b, width, height) per case)"""
    dev = [(_dev(a), _dev(b)) for _, a, b in cases]
    return dev, [(da.data_ptr() if a.size else 0, db.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for (da, db), (_, a, _) in zip(dev, cases)]


def test_compare_260_pairs_workgroups_past_their_first_tile_and_sums_beyond_32_bits():
    """With 256 or more pairs in a call an image gets 8 workgroups, whatever its size (S.grid_blocks): a workgroup then takes tile after tile over
    one LDS table, as it does in production.  Five big pairs in front -- S.trip_pairs() says what each is for --, 255 small ones behind them, most
    of whose 8 workgroups have no tile at all; then the five alone, one workgroup per tile.  The two uniform pairs sum q past -2^32 and 2^32."""
    big, want_big = S.trip_pairs(), S.trip_expected()
    fill, want_fill = S.fill_pairs(), S.fill_expected()
    n = 260
    order = [k % len(fill) for k in range(n - len(big))]
    shapes = S.TRIP_SHAPES + [fill[k][1].shape[1::-1] for k in order]
    # the preconditions, from the restated grid rule alone
    assert S.grid_blocks(n, max(S.tiles_of(*s) for s in shapes)) == 8 and n <= S.MAX_IMAGES
    assert S.trips(n, shapes, 300, 77) == [2, 1, 1, 1, 1, 1, 1, 1]                        # the full tile 0, then the corner tile 8
    assert S.trips(n, shapes, 1036, 1028) == [36] * 8 and S.trips(n, shapes, 1032, 1032) == [38] + [37] * 7
    assert S.trips(n, shapes, 517, 261) == [4] * 8 and S.trips(n, shapes, 643, 131) == [3, 3, 3, 3, 2, 2, 2, 2]
    assert S.trips(n, shapes, 12, 12) == [1, 0, 0, 0, 0, 0, 0, 0] and S.trips(n, shapes, 7, 64) == [0] * 8
    assert max(max(S.trips(len(big), S.TRIP_SHAPES, *s)) for s in S.TRIP_SHAPES) == 1   # alone: a workgroup per tile
    assert want_big[1]["sum_q16"] == [66048 * -65300] * 4 and 66048 * -65300 == -4312934400 < -(1 << 32) and want_big[1]["min_q16"] == [-65300] * 4
    assert want_big[2]["sum_q16"] == [66049 * 65536] * 4 and 66049 * 65536 > 1 << 32 and want_big[2]["min_q16"] == [65536] * 4
    keep_big, desc_big = _pair_descs(big)
    keep_fill, desc_fill = _pair_descs(fill)
    ctx = P.HipContext()
    try:
        got = ctx.compare_ssim(desc_big + [desc_fill[k] for k in order])
        alone = ctx.compare_ssim(desc_big)
    finally:
        ctx.close()
    for k, (name, _, _) in enumerate(big):
        print(name, got[k].as_dict())
        assert got[k].as_dict() == want_big[k], name
        assert alone[k].as_dict() == want_big[k], name
    assert got[2].mean(0xF) == 1.0
    for i, k in enumerate(order):
        assert got[len(big) + i].as_dict() == want_fill[k], (len(big) + i, fill[k][0])
    assert want_fill[order[2]] == want_fill[order[4]] == NO_WINDOWS                      # 7x64 and 0x0: every workgroup added nothing


def test_compare_more_pairs_than_one_launch_takes():
    """65 540 pairs: a launch takes 65 535 (S.MAX_IMAGES), so the last five are a second launch, which must start at its own jobs"""
    pool = V.split_pool()
    n = V.SPLIT_N
    assert n > S.MAX_IMAGES == 65535 and n - S.MAX_IMAGES < len(pool) == 7
    want = D.dicts_array([S.py_ssim(a, b) for _, a, b in pool], S.RECORD_DTYPE)
    assert len({w.tobytes() for w in want}) == 5                                            # (1x1, 3x1 and 0x0 have no window)
    keep, desc = _pair_descs(pool)
    ctx = P.HipContext()
    try:
        got = D.records_array(ctx.compare_ssim([desc[i % 7] for i in range(n)]), S.RECORD_DTYPE)
    finally:
        ctx.close()
    bad = D.differing(got, want[np.arange(n) % 7])
    assert not bad.size, "%d records differ, the first at %s; around the end of the first launch: %s" % (
        bad.size, bad[:8].tolist(), {i: (got[i].tolist(), want[i % 7].tolist()) for i in range(65534, 65540)})


def test_compare_refuses_a_batch_in_flight():
    import torch
    img = P.synth_rgba(160, 48, 0, 1)
    ctx = P.HipContext()
    try:
        d, f = _dev(img), torch.zeros(48, dtype=torch.uint8, device="cuda")
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), 160, 48)], 19, 2)
        out = (P.Ssim * 1)()
        pair = (L.ImagePair * 1)(L.ImagePair(d.data_ptr(), d.data_ptr(), 160, 48))
        assert P.hip_lib().pngloss_hip_compare_batch_ssim(ctx._ctx, pair, 1, out, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert P.hip_lib().pngloss_hip_last_ssim(ctx._ctx, 0, out) == L.PNGLOSS_INVALID_ARGUMENT
        ctx.finish()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the optimise path with the option on

#: (w, h, mode): both row engines (the wide one goes to the segment engine), an odd pitch, an image without windows, one without pixels
OPTION_SHAPES = [(160, 48, 0), (1536, 24, 0), (131, 69, 3), (33, 7, 5), (0, 0, 0)]


def _oracle(shape, strength=19):
    img, out, filt, rec, bpp = T.oracle_probe(*shape, strength)
    return img, out, filt, rec, S.oracle_ssim(*shape, strength)


def _run_device(ctx, imgs, strength, asynchronous):
    import torch
    dev, flt, desc = _device_batch(imgs)
    if asynchronous:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        ctx.enqueue(desc, strength, T.BLEED, stream=st.cuda_stream)
        res = ctx.finish()
        st.synchronize()
    else:
        res = ctx.run(desc, strength, T.BLEED)
    return _back(dev, flt, imgs) + (res,)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["sync", "async"])
def test_option_on_device_batches_with_and_without_distortion(asynchronous):
    ref = [_oracle(s) for s in OPTION_SHAPES]
    imgs = [r[0] for r in ref]
    ctx = P.HipContext()
    try:
        off = _run_device(ctx, imgs, 19, asynchronous)
        with pytest.raises(RuntimeError):
            ctx.ssim(0)                                 # the batch ran with the option off
        ctx.set_option("ssim", "on")
        on = _run_device(ctx, imgs, 19, asynchronous)
        recs = [ctx.ssim(i).as_dict() for i in range(len(imgs))]
        with pytest.raises(RuntimeError):
            ctx.ssim(len(imgs))
        with pytest.raises(RuntimeError):
            ctx.distortion(0)                           # independent options
        ctx.set_option("distortion", "on")
        both = _run_device(ctx, imgs, 19, asynchronous)
        recs_both = [(ctx.ssim(i).as_dict(), ctx.distortion(i).as_dict()) for i in range(len(imgs))]
        ctx.set_option("ssim", "off")
        _run_device(ctx, imgs, 19, asynchronous)
        with pytest.raises(RuntimeError):
            ctx.ssim(0)
        assert ctx.distortion(0).as_dict() == ref[0][3]
    finally:
        ctx.close()
    for i, (img, want, wf, rec, srec) in enumerate(ref):
        for run in (off, on, both):
            assert np.array_equal(run[0][i], want) and np.array_equal(run[1][i], wf), OPTION_SHAPES[i]
            assert run[2][i]["status"] == 0
        assert recs[i] == srec == S.py_ssim(img, want), OPTION_SHAPES[i]
        assert recs_both[i] == (srec, rec), OPTION_SHAPES[i]
    assert recs[3] == NO_WINDOWS and recs[4] == NO_WINDOWS and recs[0]["windows"] == 39 * 11


def test_option_on_host_batches_split_windows_and_the_multi_wrapper(monkeypatch):
    shapes = [(64, 48, 0), (130, 9, 2), (96, 64, 3), (33, 77, 4), (120, 50, 5), (257, 3, 1)]
    ref = [_oracle(s) for s in shapes]
    imgs = [r[0] for r in ref]
    wants = [r[4] for r in ref]
    assert len({tuple(w["sum_q16"]) for w in wants}) == 6                  # distinct images: a wrong chunk or context mapping shows
    lib = P.hip_lib()
    ctx = P.HipContext()
    multi = P.HipMulti("0,0")
    try:
        assert lib.pngloss_hip_set_option(ctx._ctx, b"ssim", b"maybe") == L.PNGLOSS_INVALID_ARGUMENT
        off = ctx.run_host(imgs, 19, 2)
        assert lib.pngloss_hip_last_ssim(ctx._ctx, 0, P.Ssim()) == L.PNGLOSS_INVALID_ARGUMENT
        ctx.set_option("ssim", "on")
        on = ctx.run_host(imgs, 19, 2)
        recs = [ctx.ssim(i).as_dict() for i in range(len(imgs))]
        monkeypatch.setenv("PNGLOSS_HIP_SPLIT", "2")
        split_ctx = P.HipContext()
        try:
            split_ctx.set_option("ssim", "on")
            split = split_ctx.run_host(imgs, 19, 2)
            recs_split = [split_ctx.ssim(i).as_dict() for i in range(len(imgs))]
            with pytest.raises(RuntimeError):
                split_ctx.ssim(len(imgs))
        finally:
            split_ctx.close()
        monkeypatch.delenv("PNGLOSS_HIP_SPLIT")
        assert multi.count == 2
        multi.run_host(imgs, 19, 2)
        with pytest.raises(RuntimeError):
            multi.ssim(0)                               # off by default
        multi.set_option("ssim", "on")
        multi.set_option("distortion", "on")
        mrun = multi.run_host(imgs, 19, 2)
        mrecs = [(multi.ssim(i).as_dict(), multi.distortion(i).as_dict()) for i in range(len(imgs))]
        with pytest.raises(RuntimeError):
            multi.ssim(len(imgs))
    finally:
        ctx.close()
        multi.close()
    for i, (img, want, wf, rec, srec) in enumerate(ref):
        for run in (off, on, split, mrun):
            assert np.array_equal(run[0][i], want) and np.array_equal(run[1][i], wf) and run[2][i]["status"] == 0, shapes[i]
        assert recs[i] == recs_split[i] == srec and mrecs[i] == (srec, rec), shapes[i]


# ------------------------------------------------------------------------------------------------ optimize_batch_target2

@pytest.mark.parametrize("case", TABLE["cases"], ids=lambda c: "min_ssim_%s" % c["min_ssim"])
def test_target2_strengths_equal_the_committed_table(case):
    shapes = S.TABLE_SHAPES
    imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
    ctx = P.HipContext()
    try:
        ctx.set_option("ssim", "on")                    # plays no part, and is left as it was
        dev, flt, desc = _device_batch(imgs)
        res, rep, ssim = ctx.run_target(desc, P.Target2(0.0, 0, S.TABLE_M, case["min_ssim"]), T.BLEED)
        outs, filts = _back(dev, flt, imgs)
        assert P.hip_lib().pngloss_hip_last_ssim(ctx._ctx, 0, P.Ssim()) == L.PNGLOSS_INVALID_ARGUMENT      # no single batch to index
        assert [r.strength for r in rep] == case["chosen"]
        assert [r.probes for r in rep] == [len(p) for p in case["probes"]]
        for i, (shape, img) in enumerate(zip(shapes, imgs)):
            chosen = case["chosen"][i]
            _, want, want_f, want_rec, want_bpp = T.oracle_probe(*shape, chosen)
            assert np.array_equal(outs[i], want) and np.array_equal(filts[i], want_f), shape
            assert rep[i].distortion.as_dict() == want_rec and ssim[i].as_dict() == S.oracle_ssim(*shape, chosen) == S.py_ssim(img, outs[i]), shape
            # a plain batch at that strength on a fresh copy: the same bytes, and measured, since the option is still on
            pdev, pflt, pdesc = _device_batch([img])
            plain = ctx.run(pdesc, chosen, T.BLEED)
            pouts, pfilts = _back(pdev, pflt, [img])
            assert np.array_equal(outs[i], pouts[0]) and np.array_equal(filts[i], pfilts[0]) and plain[0]["bpp"] == res[i]["bpp"] == want_bpp, shape
            assert ctx.ssim(0).as_dict() == ssim[i].as_dict()
    finally:
        ctx.close()


def test_target2_without_the_condition_is_the_older_call_and_no_window_passes_everything():
    shapes = [(64, 8, 0), (33, 16, 2), (97, 5, 1), (130, 6, 3), (0, 0, 0)]
    imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
    ctx = P.HipContext()
    try:
        dev, flt, desc = _device_batch(imgs)
        res1, rep1 = ctx.run_target(desc, P.Target(35.0, 0, 19), T.BLEED)
        out1 = _back(dev, flt, imgs)
        dev, flt, desc = _device_batch(imgs)
        res2, rep2, ssim2 = ctx.run_target(desc, P.Target2(35.0, 0, 19, 0.0), T.BLEED)
        out2 = _back(dev, flt, imgs)
        for i in range(len(imgs)):
            assert np.array_equal(out1[0][i], out2[0][i]) and np.array_equal(out1[1][i], out2[1][i])
            assert res1[i] == res2[i]
            for field in ("strength", "probes", "runs", "reserved"):
                assert getattr(rep1[i], field) == getattr(rep2[i], field), (i, field)
            assert rep1[i].distortion.as_dict() == rep2[i].distortion.as_dict()
            assert ssim2[i].as_dict() == dict(windows=0, sum_q16=[0] * 4, min_q16=[0] * 4, reserved=0)      # not filled: as the caller passed it
        # 97x5 has no window: a mean SSIM of 1.0 -- which no lossy result reaches -- does not apply to it, M is accepted; 64x8 ends at strength 0
        small = [imgs[2], imgs[0]]
        dev, flt, desc = _device_batch(small)
        res, rep, ssim = ctx.run_target(desc, P.Target2(0.0, 0, 19, 1.0), T.BLEED)
        outs, _ = _back(dev, flt, small)
        assert (rep[0].strength, rep[0].probes) == (19, 1) and np.array_equal(outs[0], T.oracle_probe(97, 5, 1, 19)[1]) and ssim[0].as_dict() == NO_WINDOWS
        assert rep[1].strength == 0 and rep[1].runs == rep[1].probes + 1 and np.array_equal(outs[1], T.oracle_probe(64, 8, 0, 0)[1])
        assert ssim[1].as_dict() == S.oracle_ssim(64, 8, 0, 0) and ssim[1].mean(0xF) == 1.0
    finally:
        ctx.close()


def test_target2_on_host_images_over_two_contexts():
    case = TABLE["cases"][0]
    shapes = S.TABLE_SHAPES
    imgs = [T.oracle_probe(w, h, mode, 0)[0] for (w, h, mode) in shapes]
    multi = P.HipMulti("0,0")
    try:
        outs, filts, res, rep, emitted, ssim = multi.run_host_target(imgs, P.Target2(0.0, 0, S.TABLE_M, case["min_ssim"]), T.BLEED, emit="scanlines")
        with pytest.raises(RuntimeError):
            multi.ssim(0)
        assert [r.strength for r in rep] == case["chosen"]
        for i, shape in enumerate(shapes):
            _, want, want_f, want_rec, want_bpp = T.oracle_probe(*shape, case["chosen"][i])
            assert np.array_equal(outs[i], want) and np.array_equal(filts[i], want_f) and res[i]["bpp"] == want_bpp, shape
            assert rep[i].distortion.as_dict() == want_rec and ssim[i].as_dict() == S.oracle_ssim(*shape, case["chosen"][i]), shape
    finally:
        multi.close()


# ------------------------------------------------------------------------------------------------ the tool

def _decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGBA"))


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers on this box)")
def test_tool_prints_the_ssim_lines_and_searches_with_target_ssim(tmp_path):
    from PIL import Image
    case = TABLE["cases"][0]
    picked = [0, 3, 5]                                  # 64x16 and 130x9 end between 0 and M, 40x7 has no window
    shapes = [S.TABLE_SHAPES[k] for k in picked]
    chosen = [case["chosen"][k] for k in picked]
    names = ["a", "b", "c"]
    src = tmp_path / "src"
    src.mkdir()
    for n, (w, h, mode) in zip(names, shapes):
        Image.fromarray(T.oracle_probe(w, h, mode, 0)[0], "RGBA").save(src / f"{n}.png")

    def run(tag, args, files):
        d = tmp_path / tag
        d.mkdir()
        for n in files:
            (d / f"{n}.png").write_bytes((src / f"{n}.png").read_bytes())
        r = subprocess.run([OUR_CLI] + args + [str(d / f"{n}.png") for n in files], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stderr[-800:])
        return [(d / f"{n}-loss.png").read_bytes() for n in files], r.stderr.splitlines()

    # --ssim on a plain run: one line per written file behind the --distortion line, the files and every other line unchanged
    plain, err_plain = run("plain", ["-s", "19", "--distortion"], names)
    got, err = run("ssim", ["-s", "19", "--distortion", "--ssim"], names)
    want_lines = []
    for shape in shapes:
        _, _, _, _, bpp = T.oracle_probe(*shape, 19)
        want_lines.append(S.cli_line(S.oracle_ssim(*shape, 19), bpp))
    assert want_lines[2] == "  ssim: not measured (smaller than one 8x8 window)" and all("mean" in x for x in want_lines[:2])
    assert got == plain and [x for x in err if x.startswith("  ssim:")] == want_lines, err
    assert [x for x in err if not x.startswith("  ssim:")] == err_plain and not [x for x in err_plain if "ssim" in x]
    for k, line in enumerate(err):
        if line.startswith("  ssim:"):
            assert err[k - 1].startswith("  distortion:")
    # --target-ssim: the strengths of the table, the files a plain -s run at those strengths writes, the lines of what was written
    got, err = run("target", ["--target-ssim", str(case["min_ssim"]), "-s", str(S.TABLE_M), "-v", "--ssim"], names)
    assert [x for x in err if x.startswith("  strength ")] == ["  strength %d chosen in %d probes" % (c, len(case["probes"][k])) for c, k in zip(chosen, picked)], err
    want_lines = []
    for n, shape, c, data in zip(names, shapes, chosen, got):
        one, _ = run(f"plain_{n}", ["-s", str(c)], [n])
        assert one[0] == data, n
        assert np.array_equal(_decode(data), T.oracle_probe(*shape, c)[1]), n
        want_lines.append(S.cli_line(S.oracle_ssim(*shape, c), T.oracle_probe(*shape, c)[4]))
    assert [x for x in err if x.startswith("  ssim:")] == want_lines
    # every set condition must hold: with a PSNR target that is stricter on this image the search ends lower
    both = S.oracle_search2((130, 9, 3), 40, 0.90, min_psnr_db=36.0)
    _, err = run("both", ["--target-ssim", "0.90", "--target-psnr", "36", "-s", "40", "-v"], ["b"])
    assert "  strength %d chosen in %d probes" % (both[0], len(both[1])) in err and both[0] == 26

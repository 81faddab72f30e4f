"""GPU tests of the visible measuring mode: pngloss_hip_compare_batch_visible on the pairs of tests/util_visible.py, in a call of 260 pairs and in one
of 65 540 (the kernels' loops past their first trip, a second launch), the option "measure" behind a batch -- of three images and of 258 -- (pixels
and filter IDs unchanged, the records those of the definition), the target search accepting on visible records, the multi-device wrapper and the
tool's --visible.

Every expected record comes from the definitions restated in numpy and Python integers (tests/util_visible.py), the optimised pixels from the CPU
oracle (U.run_port); equality is exact."""
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
NOTHING = dict(pixels=0, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)


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


def _pairs():
    """(name, a, b): the mixed shapes, the SSIM shapes and the edge pairs"""
    out = [("mixed_%dx%d" % (a.shape[1], a.shape[0]), a, b) for a, b in V.distort_pairs()]
    out += [(name, a, b) for name, (a, b) in V.ssim_pairs().items()]
    out += [(name, a, b) for name, (a, b) in V.edge_pairs().items()]
    return out


# ------------------------------------------------------------------------------------------------ compare_batch_visible

def test_compare_visible_every_pair_in_one_mixed_call():
    cases = _pairs()
    assert max(a.shape[1] * a.shape[0] for _, a, _ in cases) == 1024 * 7
    dev = [(_dev(a), _dev(b)) for _, a, b in cases]
    pairs = [(da.data_ptr() if a.size else 0, db.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for (da, db), (_, a, _) in zip(dev, cases)]
    ctx = P.HipContext()
    try:
        ctx.set_option("measure", "all")                # independent of the option, either way
        dist, ssim = ctx.compare_visible(pairs)
        ctx.set_option("measure", "visible")
        dist_only, none = ctx.compare_visible(pairs, ssim=False)
        none2, ssim_only = ctx.compare_visible(pairs, distortion=False)
        assert none is None and none2 is None and ctx.compare_visible([]) == ([], [])
        assert ctx.compare_visible(pairs, distortion=False, ssim=False) == (None, None)
        plain, plain_ssim = ctx.compare(pairs), ctx.compare_ssim(pairs)         # the two older calls stay all-pixel
    finally:
        ctx.close()
    by = {}
    for k, (name, a, b) in enumerate(cases):
        want, want_ssim = V.np_distortion(a, b), V.py_ssim(a, b)
        assert dist[k].as_dict() == dist_only[k].as_dict() == want, name
        assert ssim[k].as_dict() == ssim_only[k].as_dict() == want_ssim, name
        assert plain[k].as_dict() == D.np_distortion(a, b) and plain_ssim[k].as_dict() == S.py_ssim(a, b), name
        by[name] = (want, want_ssim, plain[k].as_dict(), plain_ssim[k].as_dict())
    assert by["invisible"][:2] == (NOTHING, V.NO_WINDOWS) and by["invisible"][2]["changed_pixels"] > 0 and by["invisible"][3]["windows"] == 5 * 3
    assert by["opaque"][0] == by["opaque"][2] and by["opaque"][1] == by["opaque"][3] and by["opaque"][1]["windows"] == 9 * 5
    assert by["alpha_0_3"][0]["pixels"] == 8 * 24 + 8 * 12 and by["alpha_0_3"][0]["max_abs"][3] == 3
    assert by["16x8_left_invisible"][1]["windows"] == 2 and by["16x8_left_invisible"][3]["windows"] == 3
    assert by["mixed_0x0"][:2] == (NOTHING, V.NO_WINDOWS) and by["7x64"][1] == V.NO_WINDOWS
    for name in ("133x37", "136x40", "137x41", "mixed_1024x7"):
        assert by[name][0] != by[name][2] and 0 < by[name][0]["pixels"] < by[name][2]["pixels"], name


def test_compare_visible_bases_off_16_byte_alignment():
    import torch
    picked = [("257x5", *V.distort_pairs()[4]), ("136x40", *V.ssim_pairs()["136x40"])]
    assert picked[0][1].shape == (5, 257, 4)
    ctx = P.HipContext()
    try:
        for name, a, b in picked:
            n = a.size
            big_a, big_b = torch.zeros(n + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
            assert big_a.data_ptr() % 16 == 0 and big_b.data_ptr() % 16 == 0
            for oa, ob in ((4, 0), (0, 12), (12, 4)):
                va, vb = big_a[oa:oa + n], big_b[ob:ob + n]
                va.copy_(torch.from_numpy(np.array(a).reshape(-1))); vb.copy_(torch.from_numpy(np.array(b).reshape(-1)))
                torch.cuda.synchronize()
                assert va.data_ptr() % 16 == oa and vb.data_ptr() % 16 == ob
                dist, ssim = ctx.compare_visible([(va.data_ptr(), vb.data_ptr(), a.shape[1], a.shape[0])])
                assert dist[0].as_dict() == V.np_distortion(a, b) and ssim[0].as_dict() == V.py_ssim(a, b), (name, oa, ob)
    finally:
        ctx.close()


def _pair_descs(cases):
    """(name, a, b) cases on the device: (the tensors, to be kept, and one (d_a, d_b, width, height) per case)"""
    dev = [(_dev(a), _dev(b)) for _, a, b in cases]
    return dev, [(da.data_ptr() if a.size else 0, db.data_ptr() if a.size else 0, a.shape[1], a.shape[0]) for (da, db), (_, a, _) in zip(dev, cases)]


def test_compare_visible_260_pairs_workgroups_past_their_first_tile():
    """The visible kernels with 8 workgroups per image (tests/test_gpu_ssim.py has the all-pixel twin and says why 260 pairs): pl_ssim_visible takes
    tile after tile over one LDS table, pl_distort_visible several quads per lane.  The noise pairs have holes and a band of invisible windows at the
    right edge; one 300 x 77 pair is invisible altogether -- every workgroup visits its tiles and must count nothing."""
    big, want_big = V.trip_pairs(), V.trip_expected()
    fill = S.fill_pairs()
    want_fill = [(V.np_distortion(a, b), V.py_ssim(a, b)) for _, a, b in fill]
    n = 260
    order = [k % len(fill) for k in range(n - len(big))]
    shapes = [a.shape[1::-1] for _, a, _ in big] + [fill[k][1].shape[1::-1] for k in order]
    assert shapes[:6] == S.TRIP_SHAPES + [(300, 77)]
    # the preconditions, from the restated grid rules alone
    assert S.grid_blocks(n, max(S.tiles_of(*s) for s in shapes)) == 8 and D.grid_blocks(n, max(w * h for w, h in shapes)) == 8
    assert S.trips(n, shapes, 300, 77) == [2, 1, 1, 1, 1, 1, 1, 1] and S.trips(n, shapes, 1036, 1028) == [36] * 8 and S.trips(n, shapes, 1032, 1032) == [38] + [37] * 7
    assert S.trips(n, shapes, 517, 261) == [4] * 8 and S.trips(n, shapes, 643, 131) == [3, 3, 3, 3, 2, 2, 2, 2]
    assert D.lane_pixels(n, 1036 * 1028, 1036 * 1028) == 4 * 131 and D.lane_pixels(n, 1036 * 1028, 517 * 261) == 4 * 17
    keep_big, desc_big = _pair_descs(big)
    keep_fill, desc_fill = _pair_descs(fill)
    ctx = P.HipContext()
    try:
        dist, ssim = ctx.compare_visible(desc_big + [desc_fill[k] for k in order])
        dist_alone, ssim_alone = ctx.compare_visible(desc_big)
    finally:
        ctx.close()
    for k, (name, a, b) in enumerate(big):
        print(name, dist[k].as_dict(), ssim[k].as_dict())
        assert (dist[k].as_dict(), ssim[k].as_dict()) == want_big[k], name
        assert (dist_alone[k].as_dict(), ssim_alone[k].as_dict()) == want_big[k], name
    assert want_big[5] == (NOTHING, V.NO_WINDOWS) and want_big[1][1]["sum_q16"][0] < -(1 << 32) and want_big[2][1]["sum_q16"][0] > 1 << 32
    for name, k in (("300x77_noise", 0), ("517x261_near", 3), ("643x131_near", 4)):
        a, b = big[k][1:]
        assert 0 < want_big[k][1]["windows"] < S.py_ssim(a, b)["windows"] and 0 < want_big[k][0]["pixels"] < a.shape[0] * a.shape[1], name
    for i, k in enumerate(order):
        assert (dist[len(big) + i].as_dict(), ssim[len(big) + i].as_dict()) == want_fill[k], (len(big) + i, fill[k][0])


def test_compare_visible_more_pairs_than_one_launch_takes():
    """65 540 pairs: a launch takes 65 535 (D.MAX_IMAGES, S.MAX_IMAGES), so the last five are a second launch of each kernel, which must start at its
    own jobs"""
    pool = V.split_pool()
    n = V.SPLIT_N
    assert n > D.MAX_IMAGES == S.MAX_IMAGES == 65535 and n - D.MAX_IMAGES < len(pool) == 7
    want_d = D.dicts_array([V.np_distortion(a, b) for _, a, b in pool])
    want_s = D.dicts_array([V.py_ssim(a, b) for _, a, b in pool], S.RECORD_DTYPE)
    assert len({w.tobytes() for w in want_d}) == 7 and want_d["pixels"].tolist()[:5] == [1, 3, 64, 144, 117] and want_d["pixels"][5] < 128
    keep, desc = _pair_descs(pool)
    ctx = P.HipContext()
    try:
        dist, ssim = ctx.compare_visible([desc[i % 7] for i in range(n)])
        got_d, got_s = D.records_array(dist), D.records_array(ssim, S.RECORD_DTYPE)
    finally:
        ctx.close()
    for what, got, want in (("distortion", got_d, want_d), ("ssim", got_s, want_s)):
        bad = D.differing(got, want[np.arange(n) % 7])
        assert not bad.size, "%s: %d records differ, the first at %s; around the end of the first launch: %s" % (
            what, bad.size, bad[:8].tolist(), {i: (got[i].tolist(), want[i % 7].tolist()) for i in range(65534, 65540)})


def test_compare_visible_refuses_a_batch_in_flight_and_bad_arguments():
    import torch
    img = P.synth_rgba(160, 48, 0, 1)
    lib = P.hip_lib()
    ctx = P.HipContext()
    try:
        d, f = _dev(img), torch.zeros(48, dtype=torch.uint8, device="cuda")
        out, sout = (P.Distortion * 1)(), (P.Ssim * 1)()
        pair = (L.ImagePair * 1)(L.ImagePair(d.data_ptr(), d.data_ptr(), 160, 48))
        assert lib.pngloss_hip_compare_batch_visible(None, pair, 1, out, sout, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_compare_batch_visible(ctx._ctx, None, 1, out, sout, None) == L.PNGLOSS_INVALID_ARGUMENT
        half = (L.ImagePair * 1)(L.ImagePair(d.data_ptr(), None, 160, 48))
        assert lib.pngloss_hip_compare_batch_visible(ctx._ctx, half, 1, out, None, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_compare_batch_visible(ctx._ctx, half, 1, None, sout, None) == L.PNGLOSS_INVALID_ARGUMENT
        ctx.enqueue([(d.data_ptr(), f.data_ptr(), 160, 48)], 19, 2)
        assert lib.pngloss_hip_compare_batch_visible(ctx._ctx, pair, 1, out, sout, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"measure", b"visible") == L.PNGLOSS_INVALID_ARGUMENT       # like every option while a batch is pending
        ctx.finish()
        assert lib.pngloss_hip_compare_batch_visible(ctx._ctx, pair, 1, out, sout, None) == L.PNGLOSS_SUCCESS
        torch.cuda.synchronize()
        now = d.cpu().numpy().reshape(img.shape)
        assert out[0].as_dict() == V.np_distortion(now, now) and sout[0].as_dict() == V.py_ssim(now, now) and out[0].changed_pixels == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the option behind a batch

def test_option_changes_the_records_and_nothing_else():
    imgs = V.batch_images()
    ref = [V.oracle_probe(i, 19) for i in range(3)]
    lib = P.hip_lib()
    ctx = P.HipContext()
    try:
        assert lib.pngloss_hip_set_option(ctx._ctx, b"measure", b"nonsense") == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"measure", b"") == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_set_option(ctx._ctx, b"measure", b"visible") == L.PNGLOSS_SUCCESS
        assert lib.pngloss_hip_set_option(ctx._ctx, b"measure", b"all") == L.PNGLOSS_SUCCESS
        ctx.set_option("measure", "visible")            # no effect while nothing measures
        dev, flt, desc = _device_batch(imgs)
        res_off = ctx.run(desc, 19, T.BLEED)
        off = _back(dev, flt, imgs)
        with pytest.raises(RuntimeError):
            ctx.distortion(0)
        ctx.set_option("distortion", "on")
        ctx.set_option("ssim", "on")
        ctx.set_option("measure", "all")
        dev, flt, desc = _device_batch(imgs)
        res_all = ctx.run(desc, 19, T.BLEED)
        all_px = _back(dev, flt, imgs)
        recs_all = [(ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) for i in range(3)]
        ctx.set_option("measure", "visible")
        dev, flt, desc = _device_batch(imgs)
        res_vis = ctx.run(desc, 19, T.BLEED)
        vis = _back(dev, flt, imgs)
        recs_vis = [(ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) for i in range(3)]
        host = ctx.run_host(imgs, 19, T.BLEED)         # the host-window path measures what the option says, too
        recs_host = [(ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) for i in range(3)]
    finally:
        ctx.close()
    # (retried_rows and repaired_pixels are diagnostics of the row engine's speculation and differ from run to run)
    for field in ("status", "bpp", "unique_symbols"):
        assert [r[field] for r in res_off] == [r[field] for r in res_all] == [r[field] for r in res_vis], field
    for i, (img, want, wf, bpp, rec, srec, vrec, vsrec) in enumerate(ref):
        for run in (off, all_px, vis, host):
            assert np.array_equal(run[0][i], want) and np.array_equal(run[1][i], wf), V.BATCH_SHAPES[i]
        assert recs_all[i] == (D.np_distortion(img, all_px[0][i]), S.py_ssim(img, all_px[0][i])) == (rec, srec), V.BATCH_SHAPES[i]
        assert recs_vis[i] == recs_host[i] == (V.np_distortion(img, vis[0][i]), V.py_ssim(img, vis[0][i])) == (vrec, vsrec), V.BATCH_SHAPES[i]
        assert vrec["pixels"] < rec["pixels"] and vsrec["windows"] < srec["windows"] and vrec != rec
        assert D.py_psnr_db(vrec, 0xF) < D.py_psnr_db(rec, 0xF)


def _transparent_corner(img):
    """a copy with its top right third made transparent white, as the transparent areas of real files are; read-only"""
    img = np.array(img)
    img[: (img.shape[0] * 2) // 3, (img.shape[1] * 2) // 3:] = (255, 255, 255, 0)
    img.setflags(write=False)
    return img


def test_options_behind_a_batch_of_258_images():
    """enqueue's own launches of pl_keep, pl_distort and pl_ssim with 8 workgroups per image at the most (256 or more images: D.grid_blocks,
    S.grid_blocks): 301 x 77 -- an odd pitch, 9 SSIM tiles on 8 workgroups, several quads per lane of pl_keep and pl_distort and a tail of one word --,
    1024 x 7 without a window, and four small images over and over.  All-pixel records, then visible ones; the pixels those of the CPU oracle and
    of the same batch with the options off."""
    distinct = [_transparent_corner(P.synth_rgba(301, 77, 0, 2)), _transparent_corner(P.synth_rgba(1024, 7, 0, 3))] + list(V.batch_images()) + [P.synth_rgba(48, 16, 5, 1)]
    ref = []
    for img in distinct:
        out, filt = U.run_port(img, 19, T.BLEED)
        ref.append((out, filt, D.np_distortion(img, out), S.py_ssim(img, out), V.np_distortion(img, out), V.py_ssim(img, out)))
    n = 258
    which = [0, 1] + [2 + k % 4 for k in range(n - 2)]
    imgs = [distinct[k] for k in which]
    shapes = [a.shape[1::-1] for a in imgs]
    # the preconditions, from the restated grid rules alone
    assert S.grid_blocks(n, max(S.tiles_of(*s) for s in shapes)) == 8 and S.trips(n, shapes, 301, 77) == [2, 1, 1, 1, 1, 1, 1, 1] and S.tiles_of(1024, 7) == 0
    assert D.grid_blocks(n, max(w * h for w, h in shapes)) == 6 and D.lane_pixels(n, 301 * 77, 301 * 77) == 16 and 301 * 77 % 4 == 1
    assert ref[0][2] != ref[0][4] and ref[0][3] != ref[0][5] and ref[0][2]["changed_pixels"] > 0          # the two modes differ on it
    ctx = P.HipContext()
    try:
        dev, flt, desc = _device_batch(imgs)
        res_off = ctx.run(desc, 19, T.BLEED)
        off = _back(dev, flt, imgs)
        ctx.set_option("distortion", "on")
        ctx.set_option("ssim", "on")
        runs = {}
        for mode in ("all", "visible"):
            ctx.set_option("measure", mode)
            dev, flt, desc = _device_batch(imgs)
            res = ctx.run(desc, 19, T.BLEED)
            runs[mode] = (_back(dev, flt, imgs), res, [(ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) for i in range(n)])
    finally:
        ctx.close()
    for i, k in enumerate(which):
        out, filt, rec, srec, vrec, vsrec = ref[k]
        assert res_off[i]["status"] == 0 and np.array_equal(off[0][i], out) and np.array_equal(off[1][i], filt), (i, shapes[i])
        for mode, want in (("all", (rec, srec)), ("visible", (vrec, vsrec))):
            (outs, filts), res, recs = runs[mode]
            assert res[i]["status"] == 0 and np.array_equal(outs[i], out) and np.array_equal(filts[i], filt), (mode, i, shapes[i])
            assert recs[i] == want, (mode, i, shapes[i])


# ------------------------------------------------------------------------------------------------ the search

def _search_wants(visible):
    wants = []
    for i in range(3):
        chosen, seq = V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, V.SEARCH_SSIM, visible)
        img, out, filt, bpp, rec, srec, vrec, vsrec = V.oracle_probe(i, chosen)
        wants.append(dict(chosen=chosen, probes=len(seq), out=out, filt=filt, bpp=bpp, rec=vrec if visible else rec, srec=vsrec if visible else srec))
    return wants


@pytest.mark.parametrize("mode", ["all", "visible"])
def test_target_search_accepts_on_the_records_of_the_mode(mode):
    imgs = V.batch_images()
    wants = _search_wants(mode == "visible")
    if mode == "visible":
        assert [w["chosen"] for w in wants] != [w["chosen"] for w in _search_wants(False)]
    ctx = P.HipContext()
    try:
        ctx.set_option("measure", mode)
        dev, flt, desc = _device_batch(imgs)
        res, rep, ssim = ctx.run_target(desc, P.Target2(V.SEARCH_PSNR, 0, V.SEARCH_M, V.SEARCH_SSIM), T.BLEED)
        outs, filts = _back(dev, flt, imgs)
    finally:
        ctx.close()
    assert [r.strength for r in rep] == [w["chosen"] for w in wants]
    assert [r.probes for r in rep] == [w["probes"] for w in wants]
    for i, w in enumerate(wants):
        assert res[i]["status"] == 0 and res[i]["bpp"] == w["bpp"]
        assert np.array_equal(outs[i], w["out"]) and np.array_equal(filts[i], w["filt"]), V.BATCH_SHAPES[i]
        assert rep[i].distortion.as_dict() == w["rec"] and ssim[i].as_dict() == w["srec"], V.BATCH_SHAPES[i]


def test_target_search_on_host_images_over_two_contexts():
    imgs = V.batch_images()
    wants = _search_wants(True)
    multi = P.HipMulti("0,0")
    try:
        multi.set_option("measure", "visible")
        outs, filts, res, rep, emitted, ssim = multi.run_host_target(imgs, P.Target2(V.SEARCH_PSNR, 0, V.SEARCH_M, V.SEARCH_SSIM), T.BLEED)
        outs1, filts1, res1, rep1, _ = multi.run_host_target(imgs, P.Target(V.SEARCH_PSNR, 0, V.SEARCH_M), T.BLEED)
    finally:
        multi.close()
    assert [r.strength for r in rep] == [w["chosen"] for w in wants]
    for i, w in enumerate(wants):
        assert np.array_equal(outs[i], w["out"]) and np.array_equal(filts[i], w["filt"]) and res[i]["bpp"] == w["bpp"], V.BATCH_SHAPES[i]
        assert rep[i].distortion.as_dict() == w["rec"] and ssim[i].as_dict() == w["srec"], V.BATCH_SHAPES[i]
        # the older call, PSNR floor alone: the replay without the SSIM condition, its record visible as well
        chosen, seq = V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, 0.0, True)
        assert (rep1[i].strength, rep1[i].probes) == (chosen, len(seq)) and rep1[i].distortion.as_dict() == V.oracle_probe(i, chosen)[6], V.BATCH_SHAPES[i]
        assert np.array_equal(outs1[i], V.oracle_probe(i, chosen)[1])


# ------------------------------------------------------------------------------------------------ the multi-device wrapper

def test_option_through_the_multi_wrapper_reaches_every_context():
    imgs = V.batch_images()
    ref = [V.oracle_probe(i, 19) for i in range(3)]
    ctx = P.HipContext()
    multi = P.HipMulti("0,0")
    try:
        assert multi.count == 2
        assert P.hip_lib().pngloss_hip_multi_set_option(multi._m, b"measure", b"nonsense") == L.PNGLOSS_INVALID_ARGUMENT
        for c in (ctx, multi):
            c.set_option("distortion", "on")
            c.set_option("ssim", "on")
            c.set_option("measure", "visible")
        one = ctx.run_host(imgs, 19, T.BLEED)
        recs_one = [(ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) for i in range(3)]
        many = multi.run_host(imgs, 19, T.BLEED)
        recs_many = [(multi.distortion(i).as_dict(), multi.ssim(i).as_dict()) for i in range(3)]
        multi.set_option("measure", "all")
        multi.run_host(imgs, 19, T.BLEED)
        recs_back = [(multi.distortion(i).as_dict(), multi.ssim(i).as_dict()) for i in range(3)]
    finally:
        ctx.close()
        multi.close()
    for i, (img, want, wf, bpp, rec, srec, vrec, vsrec) in enumerate(ref):
        assert np.array_equal(one[0][i], want) and np.array_equal(many[0][i], want) and np.array_equal(many[1][i], wf), V.BATCH_SHAPES[i]
        assert recs_one[i] == recs_many[i] == (vrec, vsrec) and recs_back[i] == (rec, srec), V.BATCH_SHAPES[i]


# ------------------------------------------------------------------------------------------------ the tool

@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers on this box)")
def test_tool_names_the_visible_counts_and_writes_the_same_file(tmp_path):
    from PIL import Image
    img = np.array(V.batch_images()[0])
    img[:, 32:] = (255, 255, 255, 0)                    # a transparent half
    (tmp_path / "plain").mkdir(); (tmp_path / "visible").mkdir()
    for tag in ("plain", "visible"):
        Image.fromarray(img, "RGBA").save(tmp_path / tag / "a.png")
    plain = subprocess.run([OUR_CLI, "-s", "19", "--distortion", "--ssim", str(tmp_path / "plain" / "a.png")], capture_output=True, text=True, timeout=300)
    vis = subprocess.run([OUR_CLI, "-s", "19", "--visible", "--distortion", "--ssim", str(tmp_path / "visible" / "a.png")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and vis.returncode == 0, (plain.stderr[-800:], vis.stderr[-800:])
    assert (tmp_path / "plain" / "a-loss.png").read_bytes() == (tmp_path / "visible" / "a-loss.png").read_bytes()
    out, _ = U.run_port(img, 19, T.BLEED)
    bpp = T.bpp_of(out)
    want = V.cli_lines(V.np_distortion(img, out), V.py_ssim(img, out), bpp)
    lines = vis.stderr.splitlines()
    assert [x for x in lines if x.startswith("  distortion") or x.startswith("  ssim")] == list(want), lines
    assert "visible pixels changed" in want[0] and " of %d visible" % int((img[..., 3] != 0).sum()) in want[0] and "windows with visible pixels" in want[1]
    assert [x for x in plain.stderr.splitlines() if x.startswith("  distortion") or x.startswith("  ssim")] == [
        D.cli_line(D.np_distortion(img, out), bpp), S.cli_line(S.py_ssim(img, out), bpp)]

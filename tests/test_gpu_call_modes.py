"""GPU tests of what a call asks of a batch (pl_host.hip: BatchCall): the searches run batches of their own that measure nothing, the byte budget
reports over all pixels, the reruns of the host forms measure what their call names -- and none of it is left behind on the context or on the peer
contexts that run the other chunks of a split host window: the plain batch that follows measures what the caller's options say.

Every expected pixel, filter ID and record comes from the CPU oracle and the definitions in numpy (tests/util_visible.py: oracle_probe); equality is
exact.  Two runs of the library are compared in one place only: the size reports under "measure" = "visible" and = "all", which have to be equal."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_target as T
from tests import util_visible as V

pytestmark = pytest.mark.gpu

STRENGTH = 19


def _target():
    return P.Target2(V.SEARCH_PSNR, 0, V.SEARCH_M, V.SEARCH_SSIM)


def _budgets(imgs):
    """three quarters of a byte per pixel: which strength that takes is the search's business, the tests hold for any"""
    return [a.shape[0] * a.shape[1] * 3 // 4 for a in imgs]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C").reshape(-1)).cuda()


def _device_batch(imgs):
    import torch
    dev = [_dev(a) for a in imgs]
    flt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
    return dev, flt, [(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)]


def _back(dev, flt, imgs):
    import torch
    torch.cuda.synchronize()
    return [d.cpu().numpy().reshape(a.shape) for d, a in zip(dev, imgs)], [f.cpu().numpy() for f in flt]


def _nothing_to_index(ctx):
    """pngloss_hip_last_* behind a search: there is no last batch"""
    lib = P.hip_lib()
    hist = np.zeros(256, np.uint32)
    assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, P.Distortion()) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_last_ssim(ctx._ctx, 0, P.Ssim()) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_last_histogram(ctx._ctx, 0, hist.ctypes.data_as(C.c_void_p)) == L.PNGLOSS_INVALID_ARGUMENT


def _size_reports_are_over_all_pixels(rep, which):
    """the record of a size report is the all-pixel record of the oracle at the strength the report names: rep[k] belongs to batch image which[k]"""
    for r, i in zip(rep, which):
        assert r.distortion.as_dict() == V.oracle_probe(i, r.strength)[4], (V.BATCH_SHAPES[i], r.as_dict())


def test_device_searches_leave_no_mode_on_the_context():
    imgs = V.batch_images()
    ref = [V.oracle_probe(i, STRENGTH) for i in range(3)]
    size_reports = {}
    ctx = P.HipContext()
    try:
        ctx.set_option("distortion", "on")
        ctx.set_option("ssim", "on")
        for mode in ("visible", "all"):
            visible = mode == "visible"
            ctx.set_option("measure", mode)
            dev, flt, desc = _device_batch(imgs)
            res, rep, ssim = ctx.run_target(desc, _target(), T.BLEED)
            _nothing_to_index(ctx)
            for i in range(3):
                chosen, seq = V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, V.SEARCH_SSIM, visible)
                probe = V.oracle_probe(i, chosen)
                assert (rep[i].strength, rep[i].probes) == (chosen, len(seq)), (mode, V.BATCH_SHAPES[i])
                assert (rep[i].distortion.as_dict(), ssim[i].as_dict()) == ((probe[6], probe[7]) if visible else (probe[4], probe[5])), (mode, V.BATCH_SHAPES[i])
            dev, flt, desc = _device_batch(imgs)
            res, rep, _ = ctx.run_size(desc, _budgets(imgs), STRENGTH, T.BLEED)
            _nothing_to_index(ctx)
            _size_reports_are_over_all_pixels(rep, range(3))
            size_reports[mode] = [r.as_dict() for r in rep]
            dev, flt, desc = _device_batch(imgs)
            res = ctx.run(desc, STRENGTH, T.BLEED)
            outs, filts = _back(dev, flt, imgs)
            for i, (img, want, wf, bpp, rec, srec, vrec, vsrec) in enumerate(ref):
                assert res[i]["status"] == 0 and np.array_equal(outs[i], want) and np.array_equal(filts[i], wf), (mode, V.BATCH_SHAPES[i])
                assert (ctx.distortion(i).as_dict(), ctx.ssim(i).as_dict()) == ((vrec, vsrec) if visible else (rec, srec)), (mode, V.BATCH_SHAPES[i])
            assert ctx.histogram(0).sum() > 0
    finally:
        ctx.close()
    assert size_reports["visible"] == size_reports["all"]
    assert all(r[6] != r[4] and r[7] != r[5] for r in ref)          # (the two modes differ on these images: a leaked mode shows)


def test_host_searches_leave_no_mode_on_peers_of_a_split_window(monkeypatch):
    monkeypatch.setenv("PNGLOSS_HIP_SPLIT", "2")
    imgs = V.batch_images() * 2
    which = [0, 1, 2] * 2
    ref = [V.oracle_probe(i, STRENGTH) for i in which]
    assert sorted(P.multi_split([(a.shape[1], a.shape[0]) for a in imgs], 2)) == [0, 0, 0, 1, 1, 1]      # three images a context: two chunks each, one on a peer
    multi, multi_all = P.HipMulti("0,0"), P.HipMulti("0,0")

    def plain_batch_measures_visible(step):
        outs, filts, res = multi.run_host(imgs, STRENGTH, T.BLEED)
        for k, (img, want, wf, bpp, rec, srec, vrec, vsrec) in enumerate(ref):
            assert res[k]["status"] == 0 and np.array_equal(outs[k], want) and np.array_equal(filts[k], wf), (step, k)
            assert (multi.distortion(k).as_dict(), multi.ssim(k).as_dict()) == (vrec, vsrec), (step, k)

    try:
        for m, mode in ((multi, "visible"), (multi_all, "all")):
            m.set_option("distortion", "on")
            m.set_option("ssim", "on")
            m.set_option("measure", mode)
        rep_size = multi.run_host_size(imgs, _budgets(imgs), STRENGTH, T.BLEED)[3]
        with pytest.raises(RuntimeError):
            multi.distortion(0)                               # a search leaves no batch to index
        plain_batch_measures_visible("behind the size search")
        outs, filts, res, rep, _, ssim = multi.run_host_target(imgs, _target(), T.BLEED)
        for k, i in enumerate(which):
            chosen, _ = V.oracle_search(i, V.SEARCH_M, V.SEARCH_PSNR, V.SEARCH_SSIM, True)
            probe = V.oracle_probe(i, chosen)
            assert rep[k].strength == chosen and np.array_equal(outs[k], probe[1]) and np.array_equal(filts[k], probe[2]), k
            assert (rep[k].distortion.as_dict(), ssim[k].as_dict()) == (probe[6], probe[7]), k
        plain_batch_measures_visible("behind the target search")
        multi.set_option("distortion", "off")
        multi.set_option("ssim", "off")
        multi.run_host_target(imgs, _target(), T.BLEED)       # (its reruns measure: its reports need the records)
        multi.run_host(imgs, STRENGTH, T.BLEED)
        for k in (0, len(imgs) - 1):
            with pytest.raises(RuntimeError):
                multi.distortion(k)
            with pytest.raises(RuntimeError):
                multi.ssim(k)
        rep_size_all = multi_all.run_host_size(imgs, _budgets(imgs), STRENGTH, T.BLEED)[3]
    finally:
        multi.close()
        multi_all.close()
    _size_reports_are_over_all_pixels(rep_size, which)
    assert [r.as_dict() for r in rep_size] == [r.as_dict() for r in rep_size_all]


SEAM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import torch
import pngloss_amd as P
data = np.load(sys.argv[1])
small = data["img2"]
def mark(text):
    sys.stderr.write(text + "\\n")
    sys.stderr.flush()
out = {}
out["on_px"], out["on_f"] = P.optimize_with_rows(small, 19, 2, verbose=True)
mark("-- verbose off --")
out["off_px"], out["off_f"] = P.optimize_with_rows(small, 19, 2)
mark("-- batch --")
imgs = [data["img0"], data["img1"]]
dev = [torch.from_numpy(a.reshape(-1).copy()).cuda() for a in imgs]
flt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
ctx = P.HipContext()
res = ctx.run([(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)], 19, 2)
torch.cuda.synchronize()
ctx.close()
assert [r["status"] for r in res] == [0, 0]
for k in range(2):
    out["px%%d" %% k], out["f%%d" %% k] = dev[k].cpu().numpy().reshape(imgs[k].shape), flt[k].cpu().numpy()
np.savez(sys.argv[2], **out)
print("seam ok")
"""


def test_the_progress_word_of_the_verbose_seam_is_not_left_on(tmp_path):
    """optimize_with_rows with -v, then without, then a plain batch, in one child process (the seam's context is the process's): every output is the
    oracle's, and between the child's two marks -- the call without -v -- nothing of the progress display is printed."""
    imgs = V.batch_images()
    ref = [V.oracle_probe(i, STRENGTH) for i in range(3)]
    assert imgs[2].shape == (8, 40, 4)
    np.savez(str(tmp_path / "in.npz"), img0=imgs[0], img1=imgs[1], img2=imgs[2])
    script = tmp_path / "seam_child.py"
    script.write_text(SEAM_CHILD % U.ROOT)
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "seam ok" in r.stdout, r.stderr[-1500:]
    verbose, rest = r.stderr.split("-- verbose off --\n")
    quiet, batch = rest.split("-- batch --\n")
    assert "compression complete" in verbose and "unique symbols" in verbose, verbose[-800:]
    for part in (quiet, batch):
        assert "complete" not in part and "unique symbols" not in part, part[-800:]
    got = np.load(str(tmp_path / "out.npz"))
    for name in ("on", "off"):
        assert np.array_equal(got[name + "_px"], ref[2][1]) and np.array_equal(got[name + "_f"], ref[2][2]), name
    for k in range(2):
        assert np.array_equal(got["px%d" % k], ref[k][1]) and np.array_equal(got["f%d" % k], ref[k][2]), k

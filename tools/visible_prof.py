"""A 4096x4096 RGBA pair with a transparent surround, measured a few times through the stand-alone calls: pngloss_hip_compare_batch and
pngloss_hip_compare_batch_ssim (kernels pl_distort and pl_ssim, every pixel) and, with the argument "both", pngloss_hip_compare_batch_visible
(kernels pl_distort_visible and pl_ssim_visible).  What `rocprofv3 --kernel-trace --stats -- python tools/visible_prof.py both` traces to set the
two modes side by side; with "all" the script runs on a library from before the visible mode as well.  Prints the
records of the last run and what the kernels read."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

W = H = 4096
MODES = sys.argv[1] if len(sys.argv) > 1 else "both"
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
assert MODES in ("all", "both")

a = P.synth_rgba(W, H, 0, 0).copy()
yy, xx = np.mgrid[0:H, 0:W]
inside = np.hypot(xx - W / 2, yy - H / 2) < W * 0.4          # about half of the frame is visible
a[..., 3] = np.where(inside, 255, 0).astype(np.uint8)
a[~inside, :3] = 255
rng = np.random.default_rng(1)
b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
b[~inside] = a[~inside]
da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
pair = [(da.data_ptr(), db.data_ptr(), W, H)]
ctx = P.HipContext()
for _ in range(RUNS):
    d, s = ctx.compare(pair)[0], ctx.compare_ssim(pair)[0]
    if MODES == "both":
        vd, vs = ctx.compare_visible(pair)
print("source_digest", P.source_digest())
print("all:     ", d.as_dict(), s.as_dict(), "PSNR %.2f dB, mean SSIM %.4f" % (d.psnr_db(0xF), s.mean(0xF)))
if MODES == "both":
    print("visible: ", vd[0].as_dict(), vs[0].as_dict(), "PSNR %.2f dB, mean SSIM %.4f" % (vd[0].psnr_db(0xF), vs[0].mean(0xF)))
    assert vd[0].pixels == int(inside.sum()) and vd[0].sq_err[3] == d.sq_err[3] and vs[0].windows < s.windows
print("bytes read per launch: %d by each of the kernels, %d runs" % (2 * a.nbytes, RUNS))
ctx.close()

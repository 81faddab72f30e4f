"""The 4096x4096 headline frame with the options "ssim" and "distortion" on, a few times, device-resident: what `rocprofv3 --kernel-trace --stats --
python tools/ssim_prof.py` traces to get the duration of pl_ssim next to pl_distort, which reads the same 128 MiB, and pl_classify, which streams
64 MiB.  Prints the record of the last run, checked against pngloss_hip_compare_batch_ssim on the same pair, and what
the three kernels moved."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

W = H = 4096
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3

frame = P.synth_rgba(W, H, 0, 0)
src = torch.from_numpy(frame).cuda()
ctx = P.HipContext()
ctx.set_option("ssim", "on")
ctx.set_option("distortion", "on")
for _ in range(RUNS):
    work = src.clone()
    filt = torch.zeros(H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = ctx.run([(work.data_ptr(), filt.data_ptr(), W, H)], 19, 2)
    assert res[0]["status"] == 0
    r, d = ctx.ssim(0), ctx.distortion(0)
again = ctx.compare_ssim([(src.data_ptr(), work.data_ptr(), W, H)])[0]
assert again.as_dict() == r.as_dict() and r.windows == 1023 * 1023
mask = P.PSNR_MASK_OF_BPP[res[0]["bpp"]]
print("source_digest", P.source_digest())
print("record:", r.as_dict(), "mean SSIM %.4f, worst window %.4f, PSNR %.2f dB" % (r.mean(mask), min(r.min_q16[c] for c in range(4) if mask >> c & 1) / 65536.0, d.psnr_db(mask)))
print("bytes per launch: pl_ssim %d (read), pl_distort %d (read), pl_classify %d (read); total_ms of the last run %.3f" % (2 * frame.nbytes, 2 * frame.nbytes, frame.nbytes, ctx.total_ms))
ctx.close()

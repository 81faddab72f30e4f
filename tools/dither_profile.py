"""Times the quantiser with and without error diffusion (pngloss_hip_quantize_batch2, include/pngloss_hip_dither.h) at N = argv[1], R = 8, on the
frame of tools/quant_profile.py: argv[2] = "single" is one 4096x4096 photograph-like frame (synth mode 0), "batch" is 256 frames of 1920x1080 (one
synthetic frame, 256 copies); argv[3] = 1 dithers, 0 takes the nearest-entry remap.  A warm-up call, then three timed ones, each on fresh copies.
Under `rocprofv3 --kernel-trace --stats -- python tools/dither_profile.py N single|batch 0|1` the kernel statistics of profiles/dither_kernels.txt
come out of the same four calls.  PNGLOSS_HIP_LIBNAME picks a variant library (PLF_MEASURE_WAVES)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

n, form, dither = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
w, h, frames = (4096, 4096, 1) if form == "single" else (1920, 1080, 256)
img = P.synth_rgba(w, h, 0, 1)
src = torch.from_numpy(img.reshape(-1)).cuda()
work = [torch.empty_like(src) for _ in range(frames)]
ctx = P.HipContext()
times = []
for k in range(4):
    for buf in work:
        buf.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, rep = ctx.quantize([(buf.data_ptr(), 0, w, h) for buf in work], n, 8, dither=dither)
    times.append((time.perf_counter() - t0) * 1e3)
r = rep[-1]
print("N", n, form, "dither", dither, "colors_in", r["colors_in"], "entries", r["entries"], "exact", r["exact"], "psnr4 %.2f dB" % P.psnr_db(r["distortion"], 0xF),
      "lib", os.environ.get("PNGLOSS_HIP_LIBNAME", "libpngloss_hip.so"))
print("N", n, form, "dither", dither, "whole call, ms: warm-up %.2f, then" % times[0], " ".join("%.2f" % t for t in times[1:]))
ctx.close()

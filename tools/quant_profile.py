"""Times pngloss_hip_quantize_batch on one 4096x4096 photograph-like frame (synth mode 0) at N = argv[1], R = 8: a warm-up call, then three timed
ones, each on a fresh copy of the frame.  Under `rocprofv3 --kernel-trace --stats -- python tools/quant_profile.py N` the kernel statistics of
profiles/quant_kernels.txt come out of the same four calls."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

n = int(sys.argv[1])
img = P.synth_rgba(4096, 4096, 0, 1)
src = torch.from_numpy(img.reshape(-1)).cuda()
work = torch.empty_like(src)
ctx = P.HipContext()
times = []
for k in range(4):
    work.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, rep = ctx.quantize([(work.data_ptr(), 0, 4096, 4096)], n, 8)
    times.append((time.perf_counter() - t0) * 1e3)
r = rep[0]
print("N", n, "colors_in", r["colors_in"], "entries", r["entries"], "exact", r["exact"], "psnr4 %.2f dB" % P.psnr_db(r["distortion"], 0xF))
print("N", n, "whole call, ms: warm-up %.2f, then" % times[0], " ".join("%.2f" % t for t in times[1:]))
ctx.close()

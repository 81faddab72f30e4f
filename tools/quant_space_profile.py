"""Times the quantiser in the two spaces of include/pngloss_hip_quant_space.h at N = argv[1], R = 8, on one 4096x4096 frame of synth_rgba mode 0 whose
alpha byte is replaced from a fixed seed: a third of the pixels 0, a third 255, a third uniform random.  argv[2] = the space: 0 or 1 call
pngloss_hip_quantize_batch3, "none" calls the older entry point (the only form a tree without the *3 calls has); argv[3] = 1 dithers; argv[4] =
"target" runs pngloss_hip_quantize_batch_target(3) at M = N with a PSNR of +inf instead: one probe at N, refused, so the measuring pass runs once
per call at exactly N.  A warm-up call, then three timed ones, each on a fresh copy.
Under `rocprofv3 --kernel-trace --stats -- python tools/quant_space_profile.py ...` the kernel statistics of profiles/quant_space_kernels.txt come
out of the same four calls."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

n, space, dither = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
target = sys.argv[4:5] == ["target"]
w = h = 4096
img = P.synth_rgba(w, h, 0, 1).copy()
rng = np.random.default_rng(73)
pick = rng.random((h, w))
img[..., 3] = np.where(pick < 1 / 3, 0, np.where(pick < 2 / 3, 255, rng.integers(0, 256, (h, w)))).astype(np.uint8)
src = torch.from_numpy(img.reshape(-1)).cuda()
work = torch.empty_like(src)
ctx = P.HipContext()
extra = {} if space == "none" else dict(space=int(space))
times = []
for k in range(4):
    work.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if target:
        _, rep = ctx.quantize_target([(work.data_ptr(), 0, w, h)], P.lib.QuantTarget(math.inf), n, 8, dither, **extra)
    else:
        _, rep = ctx.quantize([(work.data_ptr(), 0, w, h)], n, 8, dither=dither, **extra)
    times.append((time.perf_counter() - t0) * 1e3)
r = rep[-1]["quant"] if target else rep[-1]
tag = "N %d space %s dither %d%s" % (n, space, dither, " target" if target else "")
print(tag, "colors_in", r["colors_in"], "entries", r["entries"], "exact", r["exact"], "record: %d pixels, psnr4 %.2f dB" % (r["distortion"]["pixels"], P.psnr_db(r["distortion"], 0xF)))
print(tag, "whole call, ms: warm-up %.2f, then" % times[0], " ".join("%.2f" % t for t in times[1:]))
ctx.close()

"""The 4096x4096 headline frame with the option "distortion" on, a few times, device-resident: what `rocprofv3 --kernel-trace --stats -- python
tools/distort_prof.py` traces to get the durations of pl_keep and pl_distort next to pl_classify, which streams the same 64 MiB.
Prints the record of the last run and what the three kernels moved."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

W = H = 4096
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3

frame = P.synth_rgba(W, H, 0, 0)
src = torch.from_numpy(frame).cuda()
ctx = P.HipContext()
ctx.set_option("distortion", "on")
for _ in range(RUNS):
    work = src.clone()
    filt = torch.zeros(H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = ctx.run([(work.data_ptr(), filt.data_ptr(), W, H)], 19, 2)
    assert res[0]["status"] == 0
    d = ctx.distortion(0)
out = work.cpu().numpy()
diff = out.astype(np.int64) - frame.astype(np.int64)
assert d.as_dict()["sq_err"] == [int((diff[..., c] ** 2).sum()) for c in range(4)]
print("record:", d.as_dict(), "PSNR %.2f dB" % d.psnr_db(0xF))
print("bytes per launch: pl_keep %d (read + write), pl_distort %d (read), pl_classify %d (read); total_ms of the last run %.3f" % (2 * frame.nbytes, 2 * frame.nbytes, frame.nbytes, ctx.total_ms))
ctx.close()

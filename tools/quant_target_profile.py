"""Times the quantiser's colour-count search (pngloss_hip_quantize_batch_target, include/pngloss_hip_quant_target.h) against what a caller had to do
before it, on the frames of tools/dither_profile.py: argv[1] = "single" is one 4096x4096 photograph-like frame (synth mode 0), "batch" is 256 frames
of 1920x1080 (one synthetic frame, 256 copies); argv[2] = the PSNR target in dB, M = 256, R = 8; argv[3] = 1 dithers.

    call       one pngloss_hip_quantize_batch_target on fresh copies of the originals
    baseline   one pngloss_hip_quantize_batch2 per N the search probed, in its order, each on originals copied afresh (device to device: cheaper than
               the upload a caller pays), the last one at the chosen N if that was not the last probe

One warm-up of each, then three rounds of three alternated pairs (call, baseline); per round the median of each, and over the rounds the spread.
Under `rocprofv3 --kernel-trace --stats -- python tools/quant_target_profile.py single|batch DB DITHER trace` only the warm-up and ONE call run:
the kernel statistics of profiles/quant_target.txt."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

form, db, dither = sys.argv[1], float(sys.argv[2]), int(sys.argv[3])
trace = sys.argv[4:5] == ["trace"]
w, h, frames = (4096, 4096, 1) if form == "single" else (1920, 1080, 256)
img = P.synth_rgba(w, h, 0, 1)
src = torch.from_numpy(img.reshape(-1)).cuda()
work = [torch.empty_like(src) for _ in range(frames)]
descs = [(buf.data_ptr(), 0, w, h) for buf in work]
ctx = P.HipContext()
target = P.lib.QuantTarget(db)


def fresh():
    for buf in work:
        buf.copy_(src)
    torch.cuda.synchronize()


def call():
    fresh()
    t0 = time.perf_counter()
    _, rep = ctx.quantize_target(descs, target, 256, 8, dither)
    return (time.perf_counter() - t0) * 1e3, rep


def baseline(probed, chosen):
    total = 0.0
    for n in probed + ([] if probed[-1] == chosen else [chosen]):
        t0 = time.perf_counter()
        fresh()
        ctx.quantize(descs, n, 8, dither=dither)
        total += (time.perf_counter() - t0) * 1e3
    return total


warm, rep = call()
r = rep[-1]
tag = "%s %g dB dither %d" % (form, db, dither)
print(tag, "chosen", r["colors"], "reached", r["reached"], "probed", r["probed"], "mask", bin(r["accepted_mask"]), "entries", r["quant"]["entries"],
      "psnr4 %.2f dB" % P.psnr_db(r["quant"]["distortion"], 0xF), "lib", os.environ.get("PNGLOSS_HIP_LIBNAME", "libpngloss_hip.so"))
if trace:
    ms, _ = call()
    print(tag, "traced call %.2f ms (warm-up %.2f)" % (ms, warm))
else:
    baseline(r["probed"], r["colors"])
    rounds = []
    for _ in range(3):
        pairs = [(call()[0], baseline(r["probed"], r["colors"])) for _ in range(3)]
        rounds.append((statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)))
    calls, bases = [c for c, _ in rounds], [b for _, b in rounds]
    print(tag, "call, ms: warm-up %.2f, medians of three rounds" % warm, " ".join("%.2f" % c for c in calls), "(spread %.2f)" % (max(calls) - min(calls)))
    print(tag, "baseline (%d calls), ms: medians" % (len(r["probed"]) + (r["probed"][-1] != r["colors"])), " ".join("%.2f" % b for b in bases), "(spread %.2f)" % (max(bases) - min(bases)))
    print(tag, "baseline / call: %.2f" % (statistics.median(bases) / statistics.median(calls)))
ctx.close()

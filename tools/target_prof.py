"""What a strength search costs: the 4096x4096 headline frame (or, with `batch`, 32 frames of 1920x1080 as one batch) through
pngloss_hip_optimize_batch_target with M = 19, bleed 2 and a PSNR target that lands strictly inside 0..19, next to plain runs at strength 19 in the
same process.  Prints probes, runs, the wall time of the target call, the plain runs and their spread, and what the call cost beyond `runs` plain
runs.  Under `rocprofv3 --kernel-trace --stats -- python tools/target_prof.py` the trace holds pl_move next to pl_keep / pl_distort / pl_classify;
the bytes each of them moves per launch are printed at the end.

    python tools/target_prof.py [batch] [REPEATS]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

args = sys.argv[1:]
batch = bool(args) and args[0] == "batch"
if batch:
    args = args[1:]
REPEATS = int(args[0]) if args else 3
M, BLEED = 19, 2
shapes = [(1920, 1080, 0, f) for f in range(32)] if batch else [(4096, 4096, 0, 0)]
frames = [P.synth_rgba(w, h, mode, f) for (w, h, mode, f) in shapes]
src = [torch.from_numpy(a).cuda() for a in frames]
filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in frames]
ctx = P.HipContext()


def fresh():
    work = [s.clone() for s in src]
    torch.cuda.synchronize()
    return work, [(w.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for w, f, a in zip(work, filt, frames)]


def plain(strength):
    work, desc = fresh()
    t0 = time.perf_counter()
    res = ctx.run(desc, strength, BLEED)
    dt = time.perf_counter() - t0
    assert all(r["status"] == 0 for r in res)
    return dt, res


# a target strictly inside: halfway (in dB) between what strengths 9 and 19 give for the first frame
ctx.set_option("distortion", "on")
psnr = {}
for s in (9, 19):
    _, res = plain(s)
    psnr[s] = ctx.distortion(0).psnr_db(P.PSNR_MASK_OF_BPP[res[0]["bpp"]])
ctx.set_option("distortion", "off")
target_db = 0.5 * (psnr[9] + psnr[19])
print("PSNR of frame 0: strength 9 %.2f dB, strength 19 %.2f dB; target %.2f dB, M = %d" % (psnr[9], psnr[19], target_db, M))
plain_s = [plain(M)[0] for _ in range(REPEATS)]
target_s = []
for _ in range(REPEATS):
    work, desc = fresh()
    t0 = time.perf_counter()
    res, rep = ctx.run_target(desc, P.Target(target_db, 0, M), BLEED)
    target_s.append(time.perf_counter() - t0)
plain_s += [plain(M)[0] for _ in range(REPEATS)]
runs = [r.runs for r in rep]
print("chosen strengths:", sorted(set(r.strength for r in rep)), "probes", sorted(set(r.probes for r in rep)), "runs", sorted(set(runs)))
rounds = max(runs)
lo, hi = min(plain_s), max(plain_s)
print("plain run at strength %d: %s ms (spread %.1f ms)" % (M, " ".join("%.1f" % (1e3 * t) for t in plain_s), 1e3 * (hi - lo)))
print("target call: %s ms" % " ".join("%.1f" % (1e3 * t) for t in target_s))
print("target call / plain run: %.2f for %d engine rounds; beyond rounds x plain (fastest of each): %.1f ms  [the probes run at strengths below M, whose runs differ in cost]"
      % (min(target_s) / lo, rounds, 1e3 * (min(target_s) - rounds * lo)))
nbytes = sum(a.nbytes for a in frames)
print("bytes per launch over the batch: pl_move %d (read + write, one launch per round: originals saved / restored / results stashed), pl_distort %d (read), pl_classify %d (read)"
      % (2 * nbytes, 2 * nbytes, nbytes))
ctx.close()

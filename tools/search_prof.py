"""The two strength searches before and after a change of their host code (profiles/search_bookkeeping.txt): what they compute, as one digest,
and what they cost.  The library is libpngloss_hip.so, or the file PNGLOSS_HIP_LIBNAME names beside it (a build of another commit).

    python tools/search_prof.py time            64 synthetic 256x256 images (modes 0..5, frame = index), M = 19; per call one warm-up call, then ONE timed
                                                call (host clock around the synchronous call): device-form run_target with PSNR and SSIM floors, device-form
                                                run_size with budgets of a quarter of the raw scanlines and streams, and both host forms through
                                                HipMulti("0,0").  Start a fresh process per run.
    python tools/search_prof.py trace target    the five images of tests/util_target.CASES as ONE batch through the device-form target search with an SSIM
    python tools/search_prof.py trace size      condition / through the size search with streams: small, for a HIP call count under a tracer

Every call prints a digest over every output, filter list, result (without its diagnostic slot), report, SSIM record and stream."""
import ctypes as C
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

M, BLEED = 19, 2
TARGET = P.Target2(38.0, 0, M, 0.97)


def digest(*parts):
    h = hashlib.sha256()

    def feed(x):
        if x is None:
            h.update(b"-")
        elif isinstance(x, (list, tuple)):
            h.update(b"[%d" % len(x))
            for y in x:
                feed(y)
        elif isinstance(x, dict):
            feed(sorted((k, v) for k, v in x.items() if k != "repaired_pixels"))     # (a diagnostic of the run: restarts, not part of the result)
        elif isinstance(x, torch.Tensor):
            h.update(x.cpu().numpy().tobytes())
        elif isinstance(x, np.ndarray):
            h.update(np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (C.Structure, C.Array)):
            h.update(bytes(x))
        elif isinstance(x, bytes):
            h.update(x)
        else:
            h.update(repr(x).encode())

    feed(parts)
    return h.hexdigest()[:16]


def budgets(frames):
    return [max(1, (a.shape[1] * 4 + 1) * a.shape[0] // 4) for a in frames]


def device_call(ctx, frames, fn):
    work = [torch.from_numpy(a).cuda() for a in frames]
    filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in frames]
    desc = [(w.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for w, f, a in zip(work, filt, frames)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(desc)
    dt = time.perf_counter() - t0
    return 1e3 * dt, digest(work, filt, out)


def host_call(fn):
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    return 1e3 * dt, digest(out)


def main(args):
    if args[:1] == ["trace"]:
        shapes = [(64, 8, 0), (33, 16, 2), (97, 5, 1), (130, 6, 3), (64, 8, 4)]
        frames = [P.synth_rgba(w, h, mode, 0) for (w, h, mode) in shapes]
        ctx = P.HipContext()
        if args[1] == "target":
            _, d = device_call(ctx, frames, lambda desc: ctx.run_target(desc, P.Target2(35.0, 0, M, 0.9), BLEED))
        else:
            _, d = device_call(ctx, frames, lambda desc: ctx.run_size(desc, budgets(frames), M, BLEED, want_streams=True))
        ctx.close()
        print("trace %s digest %s" % (args[1], d))
        return
    frames = [P.synth_rgba(256, 256, i % 6, i) for i in range(64)]
    ctx = P.HipContext()
    calls = [("run_target", lambda: device_call(ctx, frames, lambda desc: ctx.run_target(desc, TARGET, BLEED))),
             ("run_size", lambda: device_call(ctx, frames, lambda desc: ctx.run_size(desc, budgets(frames), M, BLEED, want_streams=True)))]
    multi = P.HipMulti("0,0")
    calls += [("run_host_target", lambda: host_call(lambda: multi.run_host_target(frames, TARGET, BLEED))),
              ("run_host_size", lambda: host_call(lambda: multi.run_host_size(frames, budgets(frames), M, BLEED, emit="zlib")))]
    out = []
    for name, call in calls:
        call()
        ms, d = call()
        out.append("%s %.2f ms %s" % (name, ms, d))
    multi.close()
    ctx.close()
    print(os.environ.get("PNGLOSS_HIP_LIBNAME", "libpngloss_hip.so") + ": " + "; ".join(out))


if __name__ == "__main__":
    main(sys.argv[1:])

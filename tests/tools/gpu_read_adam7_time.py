"""Read side on the device, interlaced against non-interlaced: the SAME pixels stored as a plain PNG and as an Adam7-interlaced PNG (filter
"sub" on every row of every pass, zlib level 6), through
  (a) pngloss_hip_png_decode_batch_device     (inflated scanlines go up from page-locked memory)
  (b) pngloss_hip_png_decode_batch_device_z   (compressed bytes go up, the inflate runs on the device too)
for one 4096 x 4096 RGBA8 file and for 32 files of 1280 x 720 RGB8.  Per call: the library's own split (PNGLOSS_HIP_DEBUG_SEAM: "unfilter +
expand" is the decode kernel alone, between two stream synchronisations) and the whole call; medians over the repetitions.
usage: gpu_read_adam7_time.py [reps]"""
import ctypes as C
import os
import re
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

os.environ["PNGLOSS_HIP_DEBUG_SEAM"] = "1"            # (read when the context is created)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pngloss_amd as P  # noqa: E402
from pngloss_amd import lib as L  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
PASSES = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)


def sub_rows(px):
    """(h, w, c) uint8 -> filtered rows, filter "sub" on every row"""
    h, w, c = px.shape
    rows = px.reshape(h, w * c).astype(np.int16)
    f = rows.copy()
    f[:, c:] -= rows[:, :-c]
    return np.concatenate([np.ones((h, 1), np.uint8), (f & 255).astype(np.uint8)], axis=1).tobytes()


def png_of(px, interlace):
    h, w, c = px.shape
    if interlace:
        raw = b"".join(sub_rows(px[y0::dy, x0::dx]) for x0, y0, dx, dy in PASSES if w > x0 and h > y0)
    else:
        raw = sub_rows(px)
    ct = {3: 2, 4: 6}[c]
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ct, 0, 0, interlace)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def captured(fn):
    """runs fn with the process's stderr (the library's seam line) captured; returns (fn's result, seconds, the captured text)"""
    sys.stderr.flush()
    keep, tmp = os.dup(2), tempfile.TemporaryFile()
    os.dup2(tmp.fileno(), 2)
    try:
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
    finally:
        os.dup2(keep, 2)
        os.close(keep)
    tmp.seek(0)
    return r, dt, tmp.read().decode(errors="replace")


def main():
    lib = P.hip_lib()
    ctx = P.HipContext()
    for label, n, w, h, c, z_reps in [("1 x 4096x4096 RGBA8", 1, 4096, 4096, 4, 1), ("32 x 1280x720 RGB8", 32, 1280, 720, 3, reps)]:
        frames = [P.synth_rgba(w, h, 0, i)[:, :, :c].copy() for i in range(n)]
        for il in (0, 1):
            files = [png_of(f, il) for f in frames]
            parsed = [L.parse_png(f) for f in files]
            src, zsrc, pinned = (L.PngSource * n)(), (L.PngZSource * n)(), []
            for i, p in enumerate(parsed):
                buf = lib.pngloss_hip_pinned_alloc(len(p["scanlines"]))
                C.memmove(buf, p["scanlines"], len(p["scanlines"]))
                pinned.append(buf)
                src[i] = L.PngSource(C.cast(buf, C.c_char_p), w, h, p["ctype"], 8, None, 0, None, 0, None, interlace=il)
                zsrc[i] = L.PngZSource(p["zstream"], len(p["zstream"]), w, h, p["ctype"], 8, None, 0, None, 0, interlace=il)
            ptrs, st = (C.c_void_p * n)(), (C.c_int * n)()
            for form, call, k in (("_device", lambda: lib.pngloss_hip_png_decode_batch_device(ctx._ctx, src, n, ptrs, st, None), reps),
                                  ("_device_z", lambda: lib.pngloss_hip_png_decode_batch_device_z(ctx._ctx, zsrc, n, ptrs, st, None), z_reps)):
                if k > 1:
                    call()                                                # (workspace, frame arena, code objects; the one-stream device inflate of
                                                                          # the large file takes seconds: it runs once, and the seam split still holds)
                kern, whole = [], []
                for _ in range(k):
                    rc, dt, text = captured(call)
                    assert rc == 0 and not any(st), (label, il, form, rc, list(st))
                    kern.append(float(re.findall(r"unfilter \+ expand ([\d.]+) ms", text)[-1]))
                    whole.append(dt * 1e3)
                print("%-20s %-10s %-10s unfilter + expand %7.2f ms   whole call %8.1f ms   (%d reps)"
                      % (label, "Adam7" if il else "plain", form, float(np.median(kern)), float(np.median(whole)), k), flush=True)
            for buf in pinned:
                lib.pngloss_hip_pinned_free(buf)
    ctx.close()


if __name__ == "__main__":
    main()

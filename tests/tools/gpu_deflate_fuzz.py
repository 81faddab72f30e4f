#!/usr/bin/env python3
"""Fuzz the GPU deflate against the CPU run of the same encoder: random shapes, contents, strengths and batch mixes;
every zlib stream must (a) inflate to the emitted scanlines and (b) equal the CPU stream byte for byte.
  python tests/tools/gpu_deflate_fuzz.py SECONDS [SEED]"""
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import pngloss_amd as P  # noqa: E402
from tests import util as U  # noqa: E402


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    ctx = P.HipContext(0)
    t0 = time.time()
    images = bad = 0
    while time.time() - t0 < seconds:
        n = int(rng.integers(1, 7))
        arrays = []
        for _ in range(n):
            big = rng.random() < 0.15
            h = int(rng.integers(1, 700 if big else 60))
            w = int(rng.integers(1, 900 if big else 120))
            arrays.append(U.deflate_fuzz_content(rng, h, w)[0])
        s = int(rng.choice([0, 5, 19, 40, 85, 255]))
        b = int(rng.choice([1, 2, 8, 32767]))
        wf = bool(rng.integers(0, 2))
        outs, filts, emitted = ctx.run_host_emit(arrays, s, b, wf)
        outs2, filts2, streams = ctx.run_host_zlib(arrays, s, b, wf)
        for i in range(n):
            ctype, ids, rows = emitted[i]
            want = np.concatenate([ids[:, None], rows], axis=1).tobytes()
            zc, z, blocks = streams[i]
            ok = zc == ctype and zlib.decompress(z) == want and z == U.deflate_host(want, team=0)[0]
            images += 1
            if not ok:
                bad += 1
                print(f"MISMATCH seed {seed}: image {i} of batch, shape {arrays[i].shape}, s={s} b={b} filters={wf}", flush=True)
    print(f"deflate fuzz: {images} images in {time.time() - t0:.0f} s, {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

"""Helpers of the target tests (tests/test_target_host.py, tests/test_target_oracle.py, tests/test_gpu_target.py): the rule of
pngloss_hip_optimize_batch_target restated in Python, the fixed cases with what the CPU oracle gives for them, and the builder of the CPU harness.
Nothing here calls the code under test."""
import functools
import math
import os
import struct
import subprocess

import numpy as np

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D

BLEED = 2


def py_probe_bound(m):
    """1 + ceil(log2 M), 1 for M <= 1"""
    return 1 if m <= 1 else 1 + math.ceil(math.log2(m))


def py_search(m, accepted):
    """the rule: accepted(strength) -> bool is asked once per probe.  Returns (chosen, probe sequence)."""
    seq = [m]
    if accepted(m):
        return m, seq
    lo, hi = 0, m
    while hi - lo > 1:
        mid = (lo + hi) // 2
        seq.append(mid)
        if accepted(mid):
            lo = mid
        else:
            hi = mid
    return lo, seq


def py_accept(min_psnr_db, max_abs_error, rec, status, bpp):
    """is a probe accepted: rec = the record dict of its result against the original"""
    if status != 0:
        return False
    if rec["pixels"] == 0:
        return True
    mask = D.PSNR_MASK_OF_BPP.get(bpp, 0xF)
    if min_psnr_db != 0 and not D.py_psnr_db(rec, mask) >= min_psnr_db:
        return False
    if max_abs_error and max(rec["max_abs"][c] for c in range(4) if mask >> c & 1) > max_abs_error:
        return False
    return True


#: the fixed cases: (w, h, mode), M, min_psnr_db, max_abs_error, chosen, probe sequence -- pinned from the CPU oracle by tests/test_target_oracle.py
CASES = [
    ((64, 8, 0), 19, 35.0, 0, 13, [19, 9, 14, 11, 12, 13]),       # six probes: the bound
    ((33, 16, 2), 19, 35.0, 0, 19, [19]),                         # M accepted at once
    ((97, 5, 1), 19, 60.0, 0, 0, [19, 9, 4, 2, 1]),               # nothing accepted
    ((130, 6, 3), 40, 39.0, 0, 30, [40, 20, 30, 35, 32, 31]),     # non-monotone: 11 and 12 would fail, 20 and 30 pass
    ((64, 8, 4), 40, 0.0, 8, 8, [40, 20, 10, 5, 7, 8, 9]),        # gray, max_abs_error only
]


def bpp_of(img):
    """what pngloss_image.c:64-96 detects: 1 gray, 2 gray + alpha, 3 rgb, 4 rgba"""
    if img.size == 0:
        return 4
    gray = bool((img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all())
    opaque = bool((img[..., 3] == 255).all())
    return (1 if opaque else 2) if gray else (3 if opaque else 4)


@functools.lru_cache(maxsize=None)
def oracle_probe(w, h, mode, strength, frame=0):
    """(original, optimised pixels, row filters, record, bytes per pixel) of synth_rgba(w, h, mode, frame) at `strength`, bleed 2, from the CPU oracle
    and numpy alone; cached and read-only, so every test shares one computation"""
    img = P.synth_rgba(w, h, mode, frame)
    if img.size:
        out, filt = U.run_port(img, strength, BLEED)
    else:
        out, filt = img.copy(), np.zeros(h, np.uint8)
    rec = D.np_distortion(img, out)
    bpp = bpp_of(out)
    for a in (img, out, filt):
        a.setflags(write=False)
    return img, out, filt, rec, bpp


def oracle_search(shape, m, min_psnr_db, max_abs_error, frame=0):
    """the rule on the CPU oracle: (chosen, probe sequence, PSNR margin in dB of the closest decision or None)"""
    w, h, mode = shape
    margins = []

    def accepted(s):
        _, _, _, rec, bpp = oracle_probe(w, h, mode, s, frame)
        if min_psnr_db and rec["pixels"]:
            margins.append(abs(D.py_psnr_db(rec, D.PSNR_MASK_OF_BPP[bpp]) - min_psnr_db))
        return py_accept(min_psnr_db, max_abs_error, rec, 0, bpp)

    chosen, seq = py_search(m, accepted)
    return chosen, seq, (min(margins) if margins else None)


def double_bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def build_target_host(tmp_path):
    """tests/c/target_host.cpp with -fsanitize=address,undefined; returns the executable"""
    exe = str(tmp_path / "target_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "target_host.cpp")], check=True, capture_output=True)
    return exe


def run_target_host(exe, tmp_path, commands):
    """one answer line per command line; fails on any sanitizer report"""
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(commands) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(commands)
    return lines

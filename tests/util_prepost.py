"""Helpers of the tests of the kernels around the row engine (tests/test_prepost_host.py, tests/test_gpu_prepost.py): the numpy restatement of
original_frequency and of the rank rule, the launch shapes of pl_prepost.hip restated, the shapes and contents both test files run, and the builder
of the CPU harness (tests/c/prepost_host.cpp)."""
import functools
import os
import subprocess

import numpy as np

from tests import util as U

CLASSES = ("rgba", "rgb", "graya", "gray")
BPP_OF_CLASS = {"rgba": 4, "rgb": 3, "graya": 2, "gray": 1}
#: the channels of an RGBA image that its class keeps, in the order of the packed image (gray is the G channel)
CHANNELS_OF_BPP = {4: [0, 1, 2, 3], 3: [0, 1, 2], 2: [1, 3], 1: [1]}


def packed(img, bpp):
    """the (H, W, bpp) image the oracle takes, of an (H, W, 4) image of that class"""
    return np.ascontiguousarray(img[..., CHANNELS_OF_BPP[bpp]])


def slots(img, bpp):
    """the image as pl_repack leaves it on the device: one word per pixel, channel c of the packed image in byte c, the other bytes 0"""
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    out[..., :bpp] = packed(img, bpp)
    return out


# ---- original_frequency (optimize_state.c:66-83) and the rank rule, restated ----

def np_orig_tables(pk):
    """(5, 256) int64: over every byte of the (H, W, bpp) image, per predictor none, sub, up, average, paeth the count of (byte - prediction) mod 256,
    a neighbour outside the image being 0; numpy on whole arrays, int64"""
    h, w, _ = pk.shape
    here = pk.astype(np.int64)
    left, above, diag = np.zeros_like(here), np.zeros_like(here), np.zeros_like(here)
    left[:, 1:] = here[:, :-1]
    above[1:] = here[:-1]
    diag[1:, 1:] = here[:-1, :-1]
    p = left + above - diag
    pa, pb, pc = np.abs(p - left), np.abs(p - above), np.abs(p - diag)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, above, diag))
    preds = [np.zeros_like(here), left, above, (above + left) // 2, paeth]
    return np.stack([np.bincount(((here - pr) & 255).reshape(-1), minlength=256) for pr in preds]) if here.size else np.zeros((5, 256), np.int64)


def oracle_orig_tables(pk):
    """the same from the oracle's port_orig_histograms, (5, 256) uint32"""
    pk = np.ascontiguousarray(pk)
    h, w, bpp = pk.shape
    out = np.zeros((5, 256), np.uint32)
    U.port().port_orig_histograms(pk.ctypes.data, w, h, bpp, out.ctypes.data)
    return out


def rank_rule(freq):
    """rank[f][s] = number of s' with freq[f][s'] < freq[f][s]"""
    freq = np.asarray(freq).astype(np.int64)
    return (freq[:, None, :] < freq[:, :, None]).sum(axis=2)


# ---- the launch shapes (pl_prepost_core.h: plp_batch_blocks, plp_hist_blocks, plp_slice, PLP_MAX_IMAGES), restated ----

MAX_IMAGES, THREADS = 65535, 256
#: pl_hist as launched by default, and behind PNGLOSS_HIP_HIST=1: (threads, cap on the workgroups of a launch)
HIST_DEFAULT, HIST_VARIANT = (1024, 768), (256, 2048)


def batch_blocks(n, max_px, px_per_thread):
    """workgroups per image of pl_classify (16 pixels a thread), pl_repack and pl_unpack (8): min(needed, max(8, ceil(2048 / n))), at least 1"""
    assert n >= 1
    return max(1, min(-(-max(max_px, 1) // (THREADS * px_per_thread)), max(8, -(-2048 // n))))


def hist_blocks(n, max_px, shape=HIST_DEFAULT):
    """workgroups per image of pl_hist: a thread per 16 pixels of the largest image, min(needed, max(4, ceil(cap / n))), at least 1"""
    nt, cap = shape
    assert n >= 1
    return max(1, min(-(-max(max_px, 1) // (nt * 16)), max(4, -(-cap // n))))


def slice_images(n, first):
    return min(n - first, MAX_IMAGES)


def quad_loader(w, address, n):
    """pl_hist takes four pixels a step when rows are whole quads, the image starts on 16 bytes and its quads can be counted in 32 bits"""
    return w % 4 == 0 and address % 16 == 0 and n < 0xFFFFFFFF


def hist_trips(n, max_px, w, h, aligned=True, shape=HIST_DEFAULT):
    """(workgroups, most steps one lane of pl_hist takes) for a w x h image in a launch of n images whose largest has max_px pixels"""
    blocks = hist_blocks(n, max_px, shape)
    steps = w * h // 4 if quad_loader(w, 0 if aligned else 4, w * h) else w * h
    return blocks, -(-steps // (blocks * shape[0]))


#: the rules at the points the CPU test pins, written out: blocks for n = GRID_N
GRID_N = [1, 5, 191, 192, 256, 257, 2048, 65535]
GRID_HIST = {                                                      # max_px -> pl_hist (1024 threads, cap 768)
    0: [1] * 8, 16384: [1] * 8, 16385: [2] * 8,
    84000: [6, 6, 5, 4, 4, 4, 4, 4],                              # the capped batch of the GPU tests: six wanted, ceil(768 / 191) = 5, from 192 on four
    1 << 26: [768, 154, 5, 4, 4, 4, 4, 4],
}
GRID_BATCH16 = {                                                   # max_px -> pl_classify (256 threads, 16 pixels each)
    0: [1] * 8, 4096: [1] * 8, 4097: [2] * 8,
    1 << 26: [2048, 410, 11, 11, 8, 8, 8, 8],
}


# ---- shapes and contents ----

#: (width, height, loader of an image on 16 bytes): the smallest shapes past 16 384 pixels -- two workgroups of pl_hist, and more than one trip per lane
SHAPES = [(164, 101, "quad"), (163, 101, "scalar"), (4, 4100, "quad"), (8, 2100, "quad"), (1, 16500, "scalar"), (5464, 3, "quad"), (5465, 3, "scalar")]
FOUR_VALUES = (0, 3, 128, 255)


@functools.lru_cache(maxsize=None)
def content(w, h, kind, cls):
    """a read-only (H, W, 4) image of class cls: "noise", "four" (every byte one of FOUR_VALUES: tied and zero counts) or "flat" (one pixel value)"""
    rng = np.random.default_rng(1000 * w + h + len(kind))
    if kind == "noise":
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "four":
        img = np.array(FOUR_VALUES, np.uint8)[rng.integers(0, 4, (h, w, 4))]
    else:
        img = np.empty((h, w, 4), np.uint8)
        img[...] = (40, 90, 200, 130)
    img = U.as_pixel_class(img, cls)
    if w * h >= 1000:                                   # (the GPU tests' shapes: the device must find the class; the CPU harness is told it)
        gray = bool((img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all())
        assert (gray, bool((img[..., 3] == 255).all())) == (cls in ("graya", "gray"), cls in ("rgb", "gray")), (w, h, kind, cls)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(w, h, kind, cls, s=19, b=2, filters=True):
    """the oracle on content(w, h, kind, cls): (RGBA output, row filters, final histogram, original_frequency, ranks), read-only"""
    img = content(w, h, kind, cls)
    bpp = BPP_OF_CLASS[cls]
    pk = packed(img, bpp)
    out_pk, filt, hist = U.run_port_packed(pk, s, b, filters=filters, trace=True)
    out = np.array(img)
    out[..., CHANNELS_OF_BPP[bpp]] = out_pk
    if bpp <= 2:
        out[..., 0] = out[..., 1]; out[..., 2] = out[..., 1]
    freq = oracle_orig_tables(pk)
    res = (out, filt, hist, freq, rank_rule(freq))
    for a in res:
        if a is not None:
            a.setflags(write=False)
    return res


# ---- the CPU harness ----

def build_prepost_host(tmp_path):
    """tests/c/prepost_host.cpp with -fsanitize=address,undefined; returns the executable"""
    exe = str(tmp_path / "prepost_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "prepost_host.cpp")], check=True, capture_output=True)
    return exe


def run_host(exe, args):
    """the harness's stdout lines; fails on any sanitizer report"""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def run_cases(exe, tmp_path, cases):
    """cases: (slots image (H, W, 4), bpp, offset, blocks, threads).  Returns per case (freq (5, 256), rank (5, 256), quad loader?, pixels counted)"""
    path = str(tmp_path / "prepost_cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint64).tobytes())
        for img, bpp, off, blocks, threads in cases:
            fh.write(np.array([img.shape[1], img.shape[0], bpp, off, blocks, threads], np.uint64).tobytes())
            fh.write(np.ascontiguousarray(img).tobytes())
    lines = run_host(exe, [path])
    assert len(lines) == 3 * len(cases)
    out = []
    for k in range(len(cases)):
        freq, rank = (np.array(lines[3 * k + j].split(), np.int64).reshape(5, 256) for j in (0, 1))
        quad, pixels = (int(x) for x in lines[3 * k + 2].split())
        out.append((freq, rank, bool(quad), pixels))
    return out

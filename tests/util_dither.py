"""Helpers of the dithering tests (tests/test_dither_host.py, tests/test_gpu_dither.py): the restatement of include/pngloss_hip_dither.h as a plain
raster-order loop in Python integers on top of tests/util_quant.py (median_cut, refine, nearest) -- nothing of the kernel's schedule is in it --, the
schedule's constants restated, the shapes both suites run, and the builder of the CPU harness.  Nothing here calls the code under test for an
expected value."""
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_distort as D
from tests import util_quant as Q
from tests.util_quant import from_words, words  # noqa: F401

# pl_dither_core.h, restated (tests/test_dither_host.py holds them against the header through the harness)
LANES = 64
WAVES = 16
BAND = LANES * WAVES
K = 64
LAG = 3
RING = 256


# ---- the rule ----

def diffuse(img, palette, stats=None):
    """(H, W, 4) uint8 -> the dithered (H, W, 4) uint8 over `palette` (a list of words): raster order, the gather form.  stats: a dict that
    gets a_min and a_max, the smallest and largest a_c met."""
    h, w = img.shape[:2]
    pal = Q._channels(np.array(palette, np.uint32))              # (E, 4) int64
    rows = [[tuple(int(v) for v in px) for px in row] for row in img.tolist()]
    out = np.empty_like(img)
    zero = (0, 0, 0, 0)
    above = [zero] * (w + 2)                                    # above[x + 1] = e(y-1, x)
    a_min, a_max = 0, 255
    for y in range(h):
        cur = [zero] * (w + 2)
        left = zero
        for x in range(w):
            ul, up, ur = above[x], above[x + 1], above[x + 2]
            p = rows[y][x]
            a = [p[c] + ((7 * left[c] + ul[c] + 5 * up[c] + 3 * ur[c] + 8) >> 4) for c in range(4)]      # (>> of a Python int rounds down)
            a_min, a_max = min(a_min, *a), max(a_max, *a)
            v = [min(255, max(0, t)) for t in a]
            k = int(((pal - v) ** 2).sum(axis=1).argmin())      # the first of equals: the lowest index
            out[y, x] = pal[k]
            left = tuple(v[c] - int(pal[k, c]) for c in range(4))
            cur[x + 1] = left
        above = cur
    if stats is not None:
        stats.update(a_min=a_min, a_max=a_max)
    return out


def final_palette(img, max_colors, rounds):
    """the palette behind the refinement rounds (in the order of the median cut's list), or None for an exact image"""
    w = words(img)
    colours, counts = np.unique(w, return_counts=True)
    if len(colours) <= max_colors:
        return None
    return Q.refine(colours, counts.astype(np.int64), Q.median_cut(Q.histogram(w), max_colors), rounds)


def restate(img, max_colors, rounds=8, stats=None):
    """Q.restate's dict for the call with dither = 1: the remap step replaced by diffuse()"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    colours = np.unique(words(img))
    pal = final_palette(img, max_colors, rounds)
    if pal is None:
        out, exact = img.copy(), 1
    else:
        out, exact = diffuse(img, pal, stats), 0
    used = np.unique(words(out))
    assert len(used) <= max_colors
    return dict(pixels=out, colors_in=min(len(colours), Q.MAX_COLORS + 1), entries=len(used), exact=exact, palette=[int(x) for x in used],
                distortion=D.np_distortion(img, out))


def block_rms(a, b, block=8):
    """RMS over the four channels of the difference of the block x block means of two images (whole blocks only): what the eye integrates"""
    h, w = a.shape[0] // block * block, a.shape[1] // block * block
    mean = lambda m: m[:h, :w].astype(np.float64).reshape(h // block, block, w // block, block, 4).mean(axis=(1, 3))
    return float(np.sqrt(((mean(a) - mean(b)) ** 2).mean()))


def gradient(w=96, h=64):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return np.stack([255 * x // (w - 1), 255 * y // (h - 1), 255 * (x + y) // (w + h - 2), np.full_like(x, 255)], axis=2).astype(np.uint8)


# ---- the schedule, restated ----

def wave_epochs(w):
    return -(-(w + 2 * (LANES - 1)) // K)


def barriers(w, h):
    """barriers every wave executes for an image: per band the epochs of a wave and LAG more for every further wave with rows"""
    total = 0
    for first in range(0, h, BAND):
        rows = min(BAND, h - first)
        total += wave_epochs(w) + LAG * (-(-rows // LANES) - 1)
    return total if w else 0


# ---- the shapes ----

def shapes():
    """name -> (image, max_colors, rounds): the shapes of the issue's table, from the restated constants.  Deterministic.  Every image has more
    than max_colors colours."""
    rng = np.random.default_rng(47)
    noise = lambda w, h: from_words(rng.integers(0, 1 << 32, w * h, dtype=np.uint64).astype(np.uint32), w, h)
    inputs = U.load_npz("suite_inputs.npz")
    rose, tux = inputs["rose"], inputs["tux"]
    out = {}
    out["1x3"] = (noise(1, 3), 2, 2)                               # only the 5/16 term
    out["1x_band_plus_1"] = (noise(1, BAND + 1), 4, 2)             # a column through a band hand-over
    out["2K_plus_1_x1"] = (noise(2 * K + 1, 1), 4, 2)              # only the 7/16 term
    out["2x2"] = (noise(2, 2), 2, 2)                               # the up-right term present at x = 0 and absent at x = 1
    for w in (K - 1, K, K + 1):                                    # the epoch's edge, the hand-over from wave 0 to wave 1 at row 64
        out[f"{w}x65"] = (noise(w, LANES + 1), 8, 2)
    out["3x_two_bands_plus_1"] = (noise(3, 2 * BAND + 1), 4, 2)    # two band hand-overs through the error line; lanes with no column left
    out["3K_plus_5"] = (noise(3 * K + 5, BAND + 2), 4, 2)          # every wave past its third epoch while a band hand-over is pending
    out["ring_wraps"] = (noise(RING + 5, BAND + 2), 4, 2)          # ... and with the header's ring: it wraps while a band hand-over is pending
    for n in (3, 5, 7, 255, 16, 256):
        out[f"rose_{n}"] = (rose, n, 2 if n in (3, 5, 7, 255) else 8)
    out["tux_16"] = (tux, 16, 8)                                   # alpha that diffuses
    # both ends of the clamp: black and white pixels between entries that lie well inside
    five = np.array([0x00000000, 0xFFFFFFFF, 0x80808080, 0x40404040, 0xC0C0C0C0], np.uint32)
    out["clamp"] = (from_words(rng.choice(five, 24 * 9, p=[0.35, 0.35, 0.1, 0.1, 0.1]), 24, 9), 2, 8)
    for name, (img, n, _) in out.items():
        assert len(np.unique(words(img))) > n, name
    return out


# ---- tests/c/dither_host.cpp: the kernel's order on the CPU, under the sanitizers ----

def build_dither_host(tmp_path):
    exe = str(tmp_path / "dither_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "dither_host.cpp"), "-lpthread"], check=True, capture_output=True)
    return exe


def run_host(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def run_dither_host(exe, tmp_path, cases):
    """cases: (image (H, W, 4) uint8, palette [words], descending).  Returns per case dict(pixels, barriers, a_min, a_max); fails on any sanitizer
    report."""
    path, out_path = str(tmp_path / "dither_cases.bin"), str(tmp_path / "dither_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for img, pal, descending in cases:
            fh.write(np.array([img.shape[1], img.shape[0], len(pal), int(descending)], np.uint32).tobytes())
            fh.write(np.array(pal, np.uint32).tobytes())
            fh.write(words(img).tobytes())
    run_host(exe, ["run", path, out_path])
    raw = np.fromfile(out_path, np.uint32)
    got, at = [], 0
    for img, _, _ in cases:
        h, w = img.shape[:2]
        g = dict(pixels=from_words(raw[at:at + h * w], w, h))
        at += h * w
        g["barriers"] = int(raw[at])
        g["a_min"], g["a_max"] = (int(v) for v in raw[at + 1:at + 3].view(np.int32))
        at += 3
        got.append(g)
    assert at == raw.size
    return got

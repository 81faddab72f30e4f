"""Helpers of the premultiplied-space quantiser tests (tests/test_quant_space_host.py, tests/test_gpu_quant_space.py): include/pngloss_hip_quant_space.h
restated as a composition of what the older restatements have -- tests/util_visible.py's pm and visible-mode record, tests/util_quant.py's histogram,
median cut, refinement and nearest entry, tests/util_quant_target.py's procedure --, a plain `straight`, and a raster loop for the dithered form (the
rule of tests/util_dither.py with the alpha-0 rule); the images of the issue; and the builder of the CPU harness.  Nothing here calls the code under
test for an expected value."""
import functools
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_distort as D
from tests import util_quant as Q
from tests import util_quant_target as T
from tests import util_visible as V
from tests.util_quant import from_words, words  # noqa: F401

RGBA, VISIBLE = 0, 1


# ---- the definitions ----

def straight(e):
    """the straight word of a premultiplied palette entry"""
    e = int(e)
    a = e >> 24
    if a == 0:
        return 0
    ch = [min(255, (((e >> (8 * c)) & 255) * 255 + a // 2) // a) for c in range(3)]
    return ch[0] | ch[1] << 8 | ch[2] << 16 | a << 24


def straight_words(palette):
    return np.array([straight(e) for e in palette], np.uint32)


def pm_word(w):
    """pm of one word, in Python integers"""
    w = int(w)
    a = w >> 24
    return sum((((w >> (8 * c)) & 255) * a + 127) // 255 << (8 * c) for c in range(3)) | a << 24


def within_alpha(palette):
    """fact 2: r', g', b' <= a for every entry"""
    return all(((int(e) >> (8 * c)) & 255) <= (int(e) >> 24) for e in palette for c in range(3))


def palettes(img, max_colors, rounds):
    """(first, final): the median cut's palette of the premultiplied image and the one behind the rounds; None for an exact image (decided on the
    straight words)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if len(np.unique(words(img))) <= max_colors:
        return None
    pw = words(V.pm(img))
    colours, counts = np.unique(pw, return_counts=True)
    first = Q.median_cut(Q.histogram(pw), max_colors)
    return first, Q.refine(colours, counts.astype(np.int64), first, rounds)


def remap(img, palette):
    """every pixel p becomes straight(pal[k]), k the entry nearest to pm(p)"""
    pw = words(V.pm(img))
    colours, inverse = np.unique(pw, return_inverse=True)
    final = np.array(palette, np.uint32)
    return from_words(straight_words(final)[Q.nearest(colours, final)][inverse.reshape(-1)], img.shape[1], img.shape[0])


def diffuse(img, palette):
    """the dithered form: raster order, the gather form of tests/util_dither.py on pm(pixel) over the premultiplied entries; a pixel with alpha 0
    takes no error in; the pixel becomes straight(pal[k]) and the error stays in premultiplied units"""
    h, w = img.shape[:2]
    pal = Q._channels(np.array(palette, np.uint32))
    out_words = straight_words(palette)
    rows = [[tuple(int(v) for v in px) for px in row] for row in V.pm(img).tolist()]
    out = np.empty(h * w, np.uint32)
    zero = (0, 0, 0, 0)
    above = [zero] * (w + 2)
    for y in range(h):
        cur = [zero] * (w + 2)
        left = zero
        for x in range(w):
            ul, up, ur = above[x], above[x + 1], above[x + 2]
            p = rows[y][x]
            if p[3] == 0:
                v = [0, 0, 0, 0]
            else:
                v = [min(255, max(0, p[c] + ((7 * left[c] + ul[c] + 5 * up[c] + 3 * ur[c] + 8) >> 4))) for c in range(4)]
            k = int(((pal - v) ** 2).sum(axis=1).argmin())
            out[y * w + x] = out_words[k]
            left = tuple(v[c] - int(pal[k, c]) for c in range(4))
            cur[x + 1] = left
        above = cur
    return from_words(out, w, h)


def restate(img, max_colors, rounds=8, dither=0):
    """Q.restate's dict for the call at space 1 -- the distortion the visible-mode record --, and under "first" / "final" the premultiplied
    palettes (None for an exact image)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    colours = np.unique(words(img))
    pals = palettes(img, max_colors, rounds)
    if pals is None:
        out, exact, pals = img.copy(), 1, (None, None)
    else:
        out, exact = (diffuse if dither else remap)(img, pals[1]), 0
    used = np.unique(words(out))
    assert len(used) <= max_colors
    return dict(pixels=out, colors_in=min(len(colours), Q.MAX_COLORS + 1), entries=len(used), exact=exact, palette=[int(x) for x in used],
                distortion=V.np_distortion(img, out), first=pals[0], final=pals[1])


def visible_psnr(a, b):
    return D.py_psnr_db(V.np_distortion(a, b), 0xF)


class Probes:
    """T.Probes at space 1: at(N) is restate's dict, the search T.search over T.accepts -- which accepts a record with pixels == 0"""

    def __init__(self, img, rounds=8, dither=0):
        self.img, self.rounds, self.dither = np.ascontiguousarray(img, dtype=np.uint8), rounds, dither
        self.at = functools.lru_cache(maxsize=None)(lambda n: restate(self.img, n, self.rounds, self.dither))

    def psnr(self, n):
        return D.py_psnr_db(self.at(n)["distortion"], 0xF)

    def search(self, m, min_psnr_db=0.0, max_abs_error=0):
        out = T.search(lambda n: T.accepts(self.at(n)["distortion"], min_psnr_db, max_abs_error), m)
        out["quant"] = self.at(out["colors"])
        return out


def same_report(name, got, want):
    """a report dict of the library (QuantReport.as_dict) against restate's"""
    assert got["status"] == 0 and (got["colors_in"], got["entries"], got["exact"]) == (want["colors_in"], want["entries"], want["exact"]), (name, got, want["entries"])
    assert got["palette"] == want["palette"] and got["distortion"] == want["distortion"], (name, got["distortion"], want["distortion"])


def same_target_report(name, got, want):
    """... (QuantTargetReport.as_dict) against Probes.search's: the probe's record is the visible-mode record of the result"""
    assert (got["colors"], got["reached"], got["probes"], got["probed"], got["accepted_mask"]) == \
           (want["colors"], want["reached"], want["probes"], want["probed"], want["accepted_mask"]), (name, got, {k: v for k, v in want.items() if k != "quant"})
    same_report(name, got["quant"], want["quant"])
    assert got["probe_distortion"] == want["quant"]["distortion"], name


# ---- the images ----

@functools.lru_cache(maxsize=None)
def crop():
    """dice[192:256, 128:224]: 96x64 with 2304 transparent, 1893 partly transparent and 1947 opaque pixels, 2967 colours"""
    img = np.ascontiguousarray(U.load_npz("suite_inputs.npz")["dice"][192:256, 128:224])
    alpha = img[..., 3]
    assert img.shape == (64, 96, 4) and (int((alpha == 0).sum()), int(((alpha > 0) & (alpha < 255)).sum()), int((alpha == 255).sum())) == (2304, 1893, 1947)
    assert len(np.unique(words(img))) == 2967
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def dirty():
    """64x48: the left half alpha 0 over random RGB, the right half an opaque gradient"""
    rng = np.random.default_rng(5)
    img = np.zeros((48, 64, 4), np.uint8)
    img[:, :32, :3] = rng.integers(0, 256, (48, 32, 3))
    yy, xx = np.mgrid[0:48, 0:32]
    right = img[:, 32:]
    right[..., 0] = xx * 8
    right[..., 1] = yy * 5
    right[..., 2] = 255 - xx * 4 - yy * 2
    right[..., 3] = 255
    img.setflags(write=False)
    return img


def small_shapes():
    """name -> (image, max_colors, rounds): the small cases both suites run.  Deterministic."""
    rng = np.random.default_rng(59)
    noise = lambda w, h: from_words(rng.integers(0, 1 << 32, w * h, dtype=np.uint64).astype(np.uint32), w, h)
    out = {"1x1": (noise(1, 1), 2, 8), "1x7": (noise(1, 7), 3, 8), "5x1": (noise(5, 1), 2, 8)}
    # four invisible words that differ and three visible ones: in space 1 the four are one colour
    row = from_words(np.array([0x00112233, 0x00FFFFFF, 0x00000001, 0x00ABCDEF, 0xFF000010, 0xFF000048, 0x80FFFFFF], np.uint32), 7, 1)
    out["transparent_row_r0"] = (row, 3, 0)
    out["transparent_row_r8"] = (row, 3, 8)
    low = [c << 16 | c << 8 | c | a << 24 for a in (1, 2, 3, 254) for c in (0, 127, 128, 255)]
    out["low_alpha"] = (from_words(np.array(low, np.uint32), 16, 1), 4, 8)
    return out


def tall(seed=61):
    """3x1100 of 300 colours with random alpha: a band boundary of the dither pass with alpha-0 pixels on the error line"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, 364, dtype=np.uint64).astype(np.uint32))[:300]
    w = rng.choice(pool, 3 * 1100) | (rng.choice(np.array([0, 0, 1, 77, 200, 255], np.uint32), 3 * 1100) << 24)
    img = from_words(w.astype(np.uint32), 3, 1100)
    assert (img[1023:1026, :, 3] == 0).any()
    return img


# ---- tests/c/quant_space_host.cpp ----

def build_host(tmp_path):
    exe = str(tmp_path / "quant_space_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "quant_space_host.cpp"), "-lpthread"], check=True, capture_output=True)
    return exe


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def straight_host(exe, tmp_path):
    """plq_straight of the entry (c', c', c', a) for all 65 536 (a, c'): a (256, 256) array indexed [a, c']"""
    path = str(tmp_path / "straight.bin")
    _run(exe, ["straight", path])
    return np.fromfile(path, np.uint32).reshape(256, 256)


def run_host(exe, tmp_path, cases):
    """cases: (image, max_colors, rounds, dither, threads, descending).  Returns per case dict(pixels, first, final, record [visible pixels, changed,
    sq_err x 4, max_abs x 4]); fails on any sanitizer report."""
    path, out_path = str(tmp_path / "space_cases.bin"), str(tmp_path / "space_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for img, n, rounds, dither, threads, descending in cases:
            fh.write(np.array([img.shape[1], img.shape[0], n, rounds, dither, threads, int(descending)], np.uint32).tobytes())
            fh.write(words(img).tobytes())
    _run(exe, ["run", path, out_path])
    raw = np.fromfile(out_path, np.uint32)
    got, at = [], 0
    for img, *_ in cases:
        h, w = img.shape[:2]
        entries = int(raw[at])
        at += 1
        g = dict(first=[int(x) for x in raw[at:at + entries]], final=[int(x) for x in raw[at + entries:at + 2 * entries]])
        at += 2 * entries
        g["pixels"] = from_words(raw[at:at + h * w], w, h)
        at += h * w
        g["record"] = [int(v) for v in raw[at:at + 20].copy().view(np.uint64)]
        at += 20
        got.append(g)
    assert at == raw.size
    return got

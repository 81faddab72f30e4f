"""Helpers of the colour-quantiser tests (tests/test_quant_host.py, tests/test_gpu_quant.py): the restatement of include/pngloss_hip_quant.h in numpy
and Python integers -- histogram, median cut, refinement rounds, remap, report --, the shapes both the CPU harness and the GPU tests run, and the
builder of the CPU harness.  Nothing here calls the code under test for an expected value."""
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_distort as D
from tests.util_index import from_words, words  # noqa: F401  (re-exported: the tests build images from words)

MAX_COLORS = 256
BINS = 65536
WG_PIXELS = 1 << 24            # what one workgroup of the assign pass may take: 255 * 2^24 < 2^32
MAX_BLOCKS = 1024
MAX_PIXELS = (1 << 32) - 1     # the largest image that is taken: a histogram bin is a 32-bit count and one bin may take every pixel
CHUNK = 1024                   # pixels a workgroup takes per step: 256 lanes of 4


# ---- the definitions ----

def bin_of(w):
    """(R>>4) | (G>>4)<<4 | (B>>4)<<8 | (A>>4)<<12 of uint32 words"""
    w = np.asarray(w, np.uint32)
    return ((w >> 4) & 15) | (((w >> 12) & 15) << 4) | (((w >> 20) & 15) << 8) | (((w >> 28) & 15) << 12)


def histogram(w):
    return np.bincount(bin_of(w).astype(np.int64), minlength=BINS).astype(np.int64)


def _coord(b, c):
    return (b >> (4 * c)) & 15


def _mean(s, p):
    return (2 * int(s) + int(p)) // (2 * int(p))


def _box(bins, hist):
    """a box: its bins (ascending), its pixel count and per channel its smallest and largest coordinate"""
    return dict(bins=bins, pixels=sum(int(hist[b]) for b in bins), lo=[min(_coord(b, c) for b in bins) for c in range(4)],
                hi=[max(_coord(b, c) for b in bins) for c in range(4)])


def median_cut(hist, max_colors, trace=None):
    """the initial palette of a 65 536-bin histogram (a sequence of ints): a list of 1 .. max_colors words, in the order of the box list.
    trace: a list that gets one (box index, channel, cut) per split."""
    bins = [int(b) for b in np.nonzero(np.asarray(hist[:BINS]))[0]]          # ascending
    if not bins:
        return []
    boxes = [_box(bins, hist)]
    span = lambda box, c: box["hi"][c] - box["lo"][c]
    while len(boxes) < max_colors:
        pick = None
        for i, box in enumerate(boxes):
            if max(span(box, c) for c in range(4)) > 0 and (pick is None or box["pixels"] > boxes[pick]["pixels"]):
                pick = i
        if pick is None:
            break
        box = boxes[pick]
        spans = [span(box, c) for c in range(4)]
        ch = spans.index(max(spans))                                   # the lowest channel among equals
        lo, hi = box["lo"][ch], box["hi"][ch]
        t = hi - 1
        for v in range(lo, hi):
            if 2 * sum(int(hist[b]) for b in box["bins"] if _coord(b, ch) <= v) >= box["pixels"]:
                t = v
                break
        if trace is not None:
            trace.append((pick, ch, t))
        boxes[pick:pick + 1] = [_box([b for b in box["bins"] if _coord(b, ch) <= t], hist), _box([b for b in box["bins"] if _coord(b, ch) > t], hist)]
    out = []
    for box in boxes:
        chans = [_mean(sum(int(hist[b]) * (16 * _coord(b, c) + 8) for b in box["bins"]), box["pixels"]) for c in range(4)]
        out.append(chans[0] | chans[1] << 8 | chans[2] << 16 | chans[3] << 24)
    return out


def _channels(w):
    w = np.asarray(w, np.uint32)
    return np.stack([(w >> (8 * c)) & 255 for c in range(4)], axis=1).astype(np.int64)


def nearest(colours, palette):
    """per colour word the index of the palette entry with the smallest squared distance over the four channels; np.argmin takes the first of
    equals: the lowest index"""
    p, c = _channels(colours), _channels(palette)
    out = np.empty(len(p), np.int64)
    for a in range(0, len(p), 4096):
        d = ((p[a:a + 4096, None, :] - c[None, :, :]) ** 2).sum(axis=2)
        out[a:a + 4096] = d.argmin(axis=1)
    return out


def refine(colours, counts, palette, rounds):
    """`rounds` rounds over the distinct colours of an image and how often each occurs (sums of equal pixels are the pixel times its count)"""
    palette = [int(x) for x in palette]
    ch = _channels(colours)
    for _ in range(rounds):
        idx = nearest(colours, palette)
        for k in range(len(palette)):
            sel = idx == k
            n = int(counts[sel].sum())
            if n:
                sums = [int((ch[sel, c] * counts[sel]).sum()) for c in range(4)]
                palette[k] = _mean(sums[0], n) | _mean(sums[1], n) << 8 | _mean(sums[2], n) << 16 | _mean(sums[3], n) << 24
    return palette


def restate(img, max_colors, rounds=8):
    """dict(pixels (H, W, 4) uint8, colors_in, entries, exact, palette [ascending words in use], distortion) of an (H, W, 4) uint8 image"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w = words(img)
    colours, inverse, counts = np.unique(w, return_inverse=True, return_counts=True)
    colors_in = min(len(colours), MAX_COLORS + 1)
    if len(colours) <= max_colors:                  # (an image without pixels: 0 colours)
        out = img.copy()
        exact = 1
    else:
        first = median_cut(histogram(w), max_colors)
        final = np.array(refine(colours, counts.astype(np.int64), first, rounds), np.uint32)
        out = from_words(final[nearest(colours, final)][inverse.reshape(-1)], img.shape[1], img.shape[0])
        exact = 0
    used = np.unique(words(out))
    assert len(used) <= max_colors
    return dict(pixels=out, colors_in=colors_in, entries=len(used), exact=exact, palette=[int(x) for x in used], distortion=D.np_distortion(img, out))


def psnr4(a, b):
    """PSNR over all four channels and all pixels, in dB (inf for equal images)"""
    d = D.np_distortion(a, b)
    return D.py_psnr_db(d, 0xF)


# ---- the grid of the assign pass (pl_quant_core.h: plq_blocks, plq_wg_pixels), restated ----

def blocks(pixels, want):
    chunks = -(-pixels // CHUNK)
    need = min(-(-pixels // WG_PIXELS) * 2, MAX_BLOCKS)
    return max(1, min(max(want, need), chunks, MAX_BLOCKS))


def wg_pixels(pixels, nblocks):
    return -(-(-(-pixels // CHUNK)) // nblocks) * CHUNK


# ---- the shapes ----

def shapes():
    """name -> (image, max_colors, rounds): the shapes the issue lists.  Deterministic."""
    import pngloss_amd as P
    rng = np.random.default_rng(41)
    rose = U.load_npz("suite_inputs.npz")["rose"]
    out = {}
    out["1x1"] = (from_words([0x80123456], 1, 1), 2, 8)
    out["1x7"] = (from_words(rng.integers(0, 1 << 32, 7, dtype=np.uint64).astype(np.uint32), 1, 7), 3, 8)
    out["5x1"] = (from_words(rng.integers(0, 1 << 32, 5, dtype=np.uint64).astype(np.uint32), 5, 1), 2, 8)
    two = np.array([0xFF102030, 0xFFE0D0C0], np.uint32)
    out["3x3_two_colours_exact"] = (from_words(two[[0, 1, 1, 0, 0, 1, 1, 1, 0]], 3, 3), 2, 8)
    # three colours at N = 2, the smallest real quantisation: red 0x10 three times, 0x30 once, 0x48 three times.  The cut leaves {0x10, 0x30} and
    # {0x48}; the first round makes the entries' red 24 and 72, and from then on the pixel 0x30 = 48 is equidistant from both: the tie goes to entry 0
    out["three_colours_one_equidistant"] = (from_words(np.array([0xFF000010, 0xFF000030, 0xFF000048], np.uint32)[[0, 2, 0, 1, 2, 2, 0]], 7, 1), 2, 8)
    out["three_colours_no_rounds"] = (out["three_colours_one_equidistant"][0], 2, 0)
    out["flat_64x16"] = (from_words(np.full(64 * 16, 0xFF0A0B0C, np.uint32), 64, 16), 2, 8)
    out["rose_16"] = (rose, 16, 8)
    out["rose_256"] = (rose, 256, 8)
    out["rose_256_no_rounds"] = (rose, 256, 0)
    out["noise_257x33"] = (P.synth_rgba(257, 33, 1, 0), 256, 2)
    out["checker_64x48"] = (P.synth_rgba(64, 48, 5, 0), 4, 8)
    return out


def want_blocks(images):
    """the workgroups an image the launches of pl_quant.hip would like over `images` working images (quant_grid), restated"""
    return max(8, -(-2048 // images))


def busiest_wg_pixels(pixels, images):
    """the pixels the busiest workgroup takes of the largest image (`pixels`) of a launch over `images` working images"""
    return wg_pixels(pixels, blocks(pixels, want_blocks(images)))


def device_shapes():
    """name -> (image or list of images, max_colors, rounds): shapes for the GPU tests only -- multi-megapixel images do not belong in the CPU
    harness runs of shapes() --, at which a workgroup takes more than one chunk, a channel sum passes 2^32, the cut ends with one entry.
    Deterministic."""
    from tests.util_index import last_pixel_images
    rng = np.random.default_rng(43)
    distinct = lambda n: np.unique(rng.integers(0, 1 << 32, n + 64, dtype=np.uint64).astype(np.uint32))[:n]
    out = {}
    # 2113 chunks against the 2048 workgroups a single image gets
    pool = rng.permutation(distinct(3000))
    out["two_chunks_single"] = (from_words(rng.choice(pool, 2100 * 1030), 2100, 1030), 256, 2)
    # 256 working images: 8 workgroups each, sized by the 10 chunks of the large image in the middle
    batch = []
    for _ in range(255):
        three = distinct(3)
        batch.append(from_words(rng.permutation(three[[0, 1, 2, int(rng.integers(0, 3))]]), 2, 2))
    batch.insert(127, from_words(rng.choice(distinct(300), 100 * 100), 100, 100))
    out["two_chunks_in_a_batch"] = (batch, 2, 3)
    # one entry takes every bright pixel: its red sum is past 2^32; and the two extreme words, |c|^2 = 0 and p.c = 4 * 255^2
    three = np.array([0x00000000, 0xFFFFFFFF, 0xFFFEFDFC], np.uint32)
    out["sums_past_32_bits"] = (from_words(rng.choice(three, 4608 * 4096, p=[0.05, 0.475, 0.475]), 4608, 4096), 2, 2)
    # more than 256 colours in ONE histogram bin: the cut cannot split it
    nibbles = rng.choice(1 << 16, 299, replace=False).astype(np.uint32)
    in_one_bin = np.uint32(0x80808080) + ((nibbles & 15) | ((nibbles >> 4) & 15) << 8 | ((nibbles >> 8) & 15) << 16 | ((nibbles >> 12) & 15) << 24)
    image = from_words(rng.permutation(np.concatenate([in_one_bin, rng.choice(in_one_bin, 40 * 40 - 299)])), 40, 40)
    out["one_bin_299_colours"] = (image, 256, 8)
    out["one_bin_299_colours_to_2"] = (image, 2, 8)
    rose = U.load_npz("suite_inputs.npz")["rose"]
    for n in (3, 5, 7, 255):                                            # entry counts around the search loop's unroll of four
        out[f"rose_{n}"] = (rose, n, 2)
    for name, img in last_pixel_images().items():
        out[name] = (img, 256, 2)
    out["3x1100_300_colours"] = (from_words(rng.choice(distinct(300) | np.uint32(0xFF000000), 3 * 1100), 3, 1100), 5, 2)
    assert len(np.unique(words(out["two_chunks_single"][0]))) == 3000 and all(len(np.unique(words(a))) == 3 for a in batch if a.shape[0] == 2)
    assert len(np.unique(words(image))) == 299 and len(np.unique(bin_of(words(image)))) == 1
    return out


# ---- tests/c/quant_host.cpp: the core's bodies on the CPU, under the sanitizers ----

def build_quant_host(tmp_path):
    exe = str(tmp_path / "quant_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "quant_host.cpp"), "-lpthread"], check=True, capture_output=True)
    return exe


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def run_quant_host(exe, tmp_path, cases):
    """cases: (image (H, W, 4) uint8, max_colors, rounds, threads).  Returns per case dict(pixels, first [the median cut's palette], final [the
    palette behind the rounds], hist); fails on any sanitizer report."""
    path, out_path = str(tmp_path / "quant_cases.bin"), str(tmp_path / "quant_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for img, n, rounds, threads in cases:
            fh.write(np.array([img.shape[1], img.shape[0], n, rounds, threads], np.uint32).tobytes())
            fh.write(words(img).tobytes())
    _run(exe, ["run", path, out_path])
    raw = np.fromfile(out_path, np.uint32)
    got, at = [], 0
    for img, _, _, _ in cases:
        h, w = img.shape[:2]
        entries = int(raw[at])
        at += 1
        g = dict(first=[int(x) for x in raw[at:at + entries]], final=[int(x) for x in raw[at + entries:at + 2 * entries]])
        at += 2 * entries
        g["hist_nonzero"] = int(raw[at])
        g["hist_sum"] = int(raw[at + 1])
        at += 2
        g["pixels"] = from_words(raw[at:at + h * w], w, h)
        at += h * w
        got.append(g)
    assert at == raw.size
    return got


def cut_host(exe, tmp_path, hist, max_colors):
    """plq_median_cut on a hand-made histogram: {bin: count} -> the palette"""
    path = str(tmp_path / "hist.bin")
    full = np.zeros(BINS, np.uint32)
    for b, c in hist.items():
        full[b] = c
    full.tofile(path)
    return [int(x, 16) for x in _run(exe, ["cut", path, str(max_colors)]).split()]

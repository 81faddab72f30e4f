"""Helpers of the SSIM tests (tests/test_ssim_host.py, tests/test_ssim_oracle.py, tests/test_gpu_ssim.py): the definition of the record restated in
Python integers, the textbook float formula on the same windows, the shapes and contents both the CPU harness and the GPU tests run, the search
rule with the SSIM condition, and the builders of the CPU harnesses.  Nothing here calls the code under test."""
import functools
import json
import math
import os
import subprocess

import numpy as np

import pngloss_amd as P
from tests import util as U
from tests import util_distort as D
from tests import util_target as T

K1, K2 = 26634, 239708
ONE = 65536
#: window origins per tile of the kernel (pl_ssim_core.h: PLS_TILE_WX, PLS_TILE_WY): 128 x 32 pixels
TILE_W, TILE_H = 128, 32

#: (width, height): one window; one window and unused pixels; four windows; none (three ways); odd sizes; more than one tile in x (131 x 69 has
#: 31 x 16 windows: two tile rows); two tiles plus a partial one in both directions, windows straddling tile edges up to the last column and row;
#: no pixels
SHAPES = [(8, 8), (11, 11), (12, 12), (7, 64), (64, 7), (257, 5), (13, 9), (131, 69), (2 * TILE_W + 44, 2 * TILE_H + 13), (0, 0)]


def geometry(w, h):
    nx = (w - 8) // 4 + 1 if w >= 8 else 0
    ny = (h - 8) // 4 + 1 if h >= 8 else 0
    return (nx, ny) if nx and ny else (0, 0)


def _window_sums(x, nx, ny):
    """x: (H, W, 4) int64; the sums over the 8x8 windows at stride 4, from an integral image: (ny, nx, 4) int64"""
    h, w = x.shape[:2]
    integral = np.zeros((h + 1, w + 1, 4), np.int64)
    integral[1:, 1:] = x.cumsum(0).cumsum(1)
    ys, xs = 4 * np.arange(ny)[:, None], 4 * np.arange(nx)[None, :]
    return integral[ys + 8, xs + 8] - integral[ys, xs + 8] - integral[ys + 8, xs] + integral[ys, xs]


def _sums(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == np.uint8 and b.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4
    h, w = a.shape[:2]
    nx, ny = geometry(w, h)
    if not nx:
        return 0, 0, None
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    return nx, ny, [_window_sums(v, nx, ny) for v in (a64, b64, a64 * a64, b64 * b64, a64 * b64)]


def py_ssim(a, b):
    """the record of two (H, W, 4) uint8 arrays (b against a): the sums in numpy int64, num, den and q in Python integers"""
    nx, ny, s = _sums(a, b)
    rec = dict(windows=nx * ny, sum_q16=[0] * 4, min_q16=[ONE] * 4, reserved=0)
    if not nx:
        return rec
    sa, sb, saa, sbb, sab = (v.reshape(-1, 4).tolist() for v in s)
    for k in range(nx * ny):
        for c in range(4):
            va, vb = sa[k][c], sb[k][c]
            a1 = 2 * va * vb + K1
            b1 = va * va + vb * vb + K1
            a2 = 2 * (64 * sab[k][c] - va * vb) + K2
            b2 = 64 * (saa[k][c] + sbb[k][c]) - va * va - vb * vb + K2
            num, den = a1 * a2, b1 * b2
            assert va <= 16320 and vb <= 16320 and a1 < 2 ** 29 and b1 < 2 ** 29 and abs(a2) <= b2 < 2 ** 27.1 and abs(num) <= den < 2 ** 57
            q = (abs(num) * ONE) // den
            q = -q if num < 0 else q
            rec["sum_q16"][c] += q
            rec["min_q16"][c] = min(rec["min_q16"][c], q)
    return rec


def py_mean(rec, mask):
    """pngloss_hip_ssim_mean's formula in Python"""
    if rec["windows"] == 0 or mask == 0 or mask > 0xF:
        return math.nan
    chans = [c for c in range(4) if mask >> c & 1]
    return float(sum(rec["sum_q16"][c] for c in chans)) / (65536.0 * rec["windows"] * len(chans))


def float_ssim(a, b, mask=0xF):
    """the textbook formula in double precision on the same windows, C1 = K1 / 4096 and C2 = K2 / 4096: the mean over windows and the mask's channels"""
    nx, ny, s = _sums(a, b)
    if not nx:
        return math.nan
    sa, sb, saa, sbb, sab = (v.astype(np.float64) for v in s)
    c1, c2 = K1 / 4096.0, K2 / 4096.0
    mu_a, mu_b = sa / 64.0, sb / 64.0
    var_a, var_b, cov = saa / 64.0 - mu_a * mu_a, sbb / 64.0 - mu_b * mu_b, sab / 64.0 - mu_a * mu_b
    ssim = (2 * mu_a * mu_b + c1) * (2 * cov + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    chans = [c for c in range(4) if mask >> c & 1]
    return float(ssim[..., chans].mean())


def cli_line(rec, bpp):
    """the line `pngloss --ssim` prints for a written file"""
    if rec["windows"] == 0:
        return "  ssim: not measured (smaller than one 8x8 window)"
    mask = D.PSNR_MASK_OF_BPP[bpp]
    worst = min(rec["min_q16"][c] for c in range(4) if mask >> c & 1)
    return "  ssim: mean %.4f, worst window %.4f, %d windows" % (py_mean(rec, mask), worst / 65536.0, rec["windows"])


def contents(w, h, seed=5):
    """the hand-made pairs of a shape: name -> (a, b)"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 4, axis=2)
    half = np.repeat(((xx % 8 < 4) * 255).astype(np.uint8)[..., None], 4, axis=2)
    return {
        "equal": (noise, noise.copy()),
        "black_white": (np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8)),
        "checkerboard_inverse": (checker, 255 - checker),
        "half_inverse": (half, 255 - half),
        "noise": (noise, rng.integers(0, 256, (h, w, 4), dtype=np.uint8)),
    }


@functools.lru_cache(maxsize=None)
def oracle_pair(w, h, mode=0, strength=19, frame=0):
    """(synthetic frame, what the CPU oracle makes of it at `strength`, bleed 2, bytes per pixel of the result); cached and read-only"""
    img, out, _, _, bpp = T.oracle_probe(w, h, mode, strength, frame)
    return img, out, bpp


@functools.lru_cache(maxsize=None)
def oracle_ssim(w, h, mode, strength, frame=0):
    img, out, _ = oracle_pair(w, h, mode, strength, frame)
    return py_ssim(img, out)


def all_cases():
    """every (name, a, b) the CPU harness and the GPU compare: each shape with each content, and the oracle's result on a synthetic frame"""
    out = []
    for w, h in SHAPES:
        for name, (a, b) in contents(w, h).items():
            out.append(("%dx%d_%s" % (w, h, name), a, b))
        if w and h:
            img, res, _ = oracle_pair(w, h, 0, 19)
            out.append(("%dx%d_oracle" % (w, h), img, res))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """py_ssim of a case of all_cases(), computed once per process"""
    for n, a, b in all_cases():
        if n == name:
            return py_ssim(a, b)
    raise KeyError(name)


# ---- the pairs that take a workgroup of pl_ssim past its first tile, and sum_q16 past 32 bits ----

#: (width, height) of the five big pairs; with 256 or more pairs in a call an image gets 8 workgroups (grid_blocks), which then take
#: 9 tiles (a full one, then the partial corner in workgroup 0); 288 tiles = 36 each; 297 = 37 and a remainder; 32 full tiles = 4 each; 20 = 3 or 2 each
TRIP_SHAPES = [(300, 77), (1036, 1028), (1032, 1032), (517, 261), (643, 131)]
#: the shapes of the small pairs that fill such a call: one window, four, none, two, no pixels
FILL_SHAPES = [(8, 8), (12, 12), (7, 64), (13, 9), (0, 0)]


def near_pair(w, h, seed):
    """noise and the same noise +- 12"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return a, np.clip(a.astype(np.int64) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def trip_pairs():
    """[(name, a, b)] of TRIP_SHAPES, read-only: noise against noise; a checkerboard against its inverse (every window the same 8x8 pair); equal
    images; noise against noise +- 12 on an odd width (word-by-word loads) whose 128 x 64 windows fill 32 tiles to the brim; the same on 159 x 31
    windows, 5 x 4 tiles partial in both directions"""
    out = [("300x77_noise",) + contents(300, 77)["noise"], ("1036x1028_checkerboard_inverse",) + contents(1036, 1028)["checkerboard_inverse"],
           ("1032x1032_equal",) + contents(1032, 1032)["equal"], ("517x261_near",) + near_pair(517, 261, 41), ("643x131_near",) + near_pair(643, 131, 43)]
    assert [(a.shape[1], a.shape[0]) for _, a, _ in out] == TRIP_SHAPES
    for _, a, b in out:
        a.setflags(write=False); b.setflags(write=False)
    return out


def uniform_record(a, b, ssim=None):
    """the record of a pair whose windows are all the 8x8 pair at its top left corner -- a pattern of period 4 or less both ways, or equal images --:
    the corner's q, times the window count.  (tests/test_ssim_host.py checks it against py_ssim on the whole pair.)"""
    nx, ny = geometry(a.shape[1], a.shape[0])
    one = (ssim or py_ssim)(a[:8, :8], b[:8, :8])
    assert one["windows"] == 1 and one["sum_q16"] == one["min_q16"]
    return dict(windows=nx * ny, sum_q16=[nx * ny * q for q in one["sum_q16"]], min_q16=one["min_q16"], reserved=0)


@functools.lru_cache(maxsize=None)
def trip_expected():
    """the records of trip_pairs(): py_ssim, but for the two uniform pairs of 66 048 and 66 049 windows, which have a closed form"""
    return [uniform_record(a, b) if name in ("1036x1028_checkerboard_inverse", "1032x1032_equal") else py_ssim(a, b) for name, a, b in trip_pairs()]


@functools.lru_cache(maxsize=None)
def fill_pairs():
    """[(name, a, b)]: every content of every shape of FILL_SHAPES, shape by shape in turn"""
    by = {s: list(contents(*s).items()) for s in FILL_SHAPES}
    return [("%dx%d_%s" % (s + (by[s][k][0],)),) + by[s][k][1] for k in range(5) for s in FILL_SHAPES]


@functools.lru_cache(maxsize=None)
def fill_expected():
    return [py_ssim(a, b) for _, a, b in fill_pairs()]


#: PlSsimRecord / pngloss_hip_ssim as a numpy record (D.records_array, D.dicts_array)
RECORD_DTYPE = np.dtype([("windows", "<u8"), ("sum_q16", "<i8", (4,)), ("min_q16", "<i4", (4,)), ("reserved", "<u8")])


# ---- the launch shape of pl_ssim (pl_ssim_core.h: pls_grid_blocks, PLS_MAX_IMAGES), restated ----

#: a launch takes at most this many images; a larger batch is launched in slices
MAX_IMAGES = 65535


def grid_blocks(n, max_tiles):
    """workgroups per image of a launch of n images whose largest has max_tiles tiles: min(max_tiles, max(8, ceil(2048 / n))), at least 1"""
    assert n >= 1
    return max(1, min(max_tiles, max(8, -(-2048 // n))))


#: the rule at the points the CPU test pins, written out: {max_tiles: blocks for n = GRID_N}
GRID_N = [1, 5, 59, 255, 256, 257, 300, 65535]
GRID_POINTS = {
    0: [1, 1, 1, 1, 1, 1, 1, 1],
    1: [1, 1, 1, 1, 1, 1, 1, 1],
    8: [8, 8, 8, 8, 8, 8, 8, 8],
    9: [9, 9, 9, 9, 8, 8, 8, 8],
    288: [288, 288, 35, 9, 8, 8, 8, 8],
    4096: [2048, 410, 35, 9, 8, 8, 8, 8],
}


def tiles_of(w, h):
    nx, ny = geometry(w, h)
    return -(-nx // 32) * -(-ny // 8)


def trips(n, shapes, w, h):
    """how many tiles each workgroup of a w x h image takes in a launch of n images whose sizes are `shapes` ((w, h) each): one count per workgroup"""
    blocks = grid_blocks(n, max(tiles_of(*s) for s in shapes))
    return [len(range(b, tiles_of(w, h), blocks)) for b in range(blocks)]


def run_ssim_grid(exe, points):
    """points: (n, max_tiles) each.  Returns (PLS_MAX_IMAGES, [pls_grid_blocks(n, max_tiles)]) from the C code"""
    lines = _run(exe, ["grid"] + [str(v) for p in points for v in p], len(points) + 1)
    return int(lines[0]), [int(x) for x in lines[1:]]


# ---- the search with the SSIM condition (pngloss_hip_optimize_batch_target2) ----

def py_accept2(min_psnr_db, max_abs_error, min_ssim, rec, srec, status, bpp):
    """is a probe accepted: rec / srec = the distortion and SSIM record dicts of its result against the original"""
    if not T.py_accept(min_psnr_db, max_abs_error, rec, status, bpp):
        return False
    if min_ssim == 0 or srec["windows"] == 0 or rec["pixels"] == 0:
        return True
    return py_mean(srec, D.PSNR_MASK_OF_BPP.get(bpp, 0xF)) >= min_ssim


def oracle_search2(shape, m, min_ssim, min_psnr_db=0.0, max_abs_error=0, frame=0):
    """the rule on the CPU oracle: (chosen, probe sequence, margin of the closest SSIM decision or None)"""
    w, h, mode = shape
    margins = []

    def accepted(s):
        _, _, _, rec, bpp = T.oracle_probe(w, h, mode, s, frame)
        srec = oracle_ssim(w, h, mode, s, frame)
        if min_ssim and srec["windows"]:
            margins.append(abs(py_mean(srec, D.PSNR_MASK_OF_BPP[bpp]) - min_ssim))
        return py_accept2(min_psnr_db, max_abs_error, min_ssim, rec, srec, 0, bpp)

    chosen, seq = T.py_search(m, accepted)
    return chosen, seq, (min(margins) if margins else None)


#: the images of the committed table (tests/golden/ssim_target_table.json): (w, h, mode), all at M = 40, bleed 2
TABLE_SHAPES = [(64, 16, 0), (33, 16, 2), (97, 12, 1), (130, 9, 3), (64, 8, 4), (40, 7, 0)]
TABLE_M = 40
TABLE_PATH = os.path.join(U.ROOT, "tests", "golden", "ssim_target_table.json")


def load_table():
    with open(TABLE_PATH) as fh:
        return json.load(fh)


# ---- the CPU harnesses ----

def _build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", name + ".cpp")], check=True, capture_output=True)
    return exe


def build_ssim_host(tmp_path):
    """tests/c/ssim_host.cpp with -fsanitize=address,undefined (as D.build_distort_host builds its harness); returns the executable"""
    return _build(tmp_path, "ssim_host")


def build_target2_host(tmp_path):
    """tests/c/target2_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "target2_host")


def _run(exe, args, n):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == n
    return lines


def run_ssim_host(exe, tmp_path, cases):
    """cases: (a, b, a_offset, b_offset, nthreads[, blocks[, visible]]) with a, b (H, W, 4) uint8; blocks = B > 0 runs the tiles as B workgroups
    of the kernel would, each over one table that is never cleared between its tiles, visible = 1 the visible instantiation
    (tests/c/ssim_host.cpp).  Returns one record dict per case; fails on any sanitizer report."""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint64).tobytes())
        for a, b, oa, ob, nt, *more in cases:
            blocks, visible = (list(more) + [0, 0])[:2]
            fh.write(np.array([a.shape[1], a.shape[0], oa, ob, nt, blocks, visible], np.uint64).tobytes())
            fh.write(np.ascontiguousarray(a).tobytes())
            fh.write(np.ascontiguousarray(b).tobytes())
    recs = []
    for line in _run(exe, [path], len(cases)):
        v = [int(x) for x in line.split()]
        recs.append(dict(windows=v[0], sum_q16=v[1:5], min_q16=v[5:9], reserved=v[9]))
    return recs


def run_target2_host(exe, tmp_path, commands):
    """one answer line per command line; fails on any sanitizer report"""
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(commands) + "\n")
    return _run(exe, [path], len(commands))

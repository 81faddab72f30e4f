"""Helpers of the visible-mode tests (tests/test_visible_host.py, tests/test_gpu_visible.py): the definitions of include/pngloss_hip.h ("Measuring over
visible pixels") restated in numpy and Python integers -- pm, the visible masks, the two records, the window rule --, the images and pairs both the
CPU harness and the GPU tests run, the target search replayed on the CPU oracle with visible records, and the builder of the CPU harness.
Nothing here calls the code under test."""
import functools
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_distort as D
from tests import util_ssim as S
from tests import util_target as T

ONE = S.ONE
NO_WINDOWS = dict(windows=0, sum_q16=[0] * 4, min_q16=[ONE] * 4, reserved=0)


def pm(x):
    """the premultiplied image of an (..., 4) uint8 array: alpha kept, each of R, G, B the integer nearest to c * A / 255"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.uint8 and x.shape[-1] == 4
    out = x.copy()
    alpha = x[..., 3:4].astype(np.int64)
    out[..., :3] = (x[..., :3].astype(np.int64) * alpha + 127) // 255
    return out


def visible_mask(a, b):
    """(H, W) bool: alpha non-zero in a or in b"""
    return (a[..., 3] != 0) | (b[..., 3] != 0)


def np_distortion(a, b):
    """the distortion record in visible mode of two (H, W, 4) uint8 arrays (b against a)"""
    rec = D.np_distortion(pm(a), pm(b))
    rec["pixels"] = int(visible_mask(a, b).sum())
    return rec


def py_ssim(a, b):
    """the SSIM record in visible mode: the window arithmetic of S.py_ssim restated on pm(a), pm(b), over the windows that hold a visible pixel"""
    pa, pb = pm(a), pm(b)
    nx, ny, s = S._sums(pa, pb)
    rec = dict(windows=0, sum_q16=[0] * 4, min_q16=[ONE] * 4, reserved=0)
    if not nx:
        return rec
    seen = S._window_sums(np.repeat(visible_mask(a, b)[..., None], 4, axis=2).astype(np.int64), nx, ny)[..., 0].reshape(-1).tolist()
    sa, sb, saa, sbb, sab = (v.reshape(-1, 4).tolist() for v in s)
    for k in range(nx * ny):
        if not seen[k]:
            continue
        rec["windows"] += 1
        for c in range(4):
            va, vb = sa[k][c], sb[k][c]
            num = (2 * va * vb + S.K1) * (2 * (64 * sab[k][c] - va * vb) + S.K2)
            den = (va * va + vb * vb + S.K1) * (64 * (saa[k][c] + sbb[k][c]) - va * va - vb * vb + S.K2)
            assert abs(num) <= den < 2 ** 57
            q = (abs(num) * ONE) // den
            q = -q if num < 0 else q
            rec["sum_q16"][c] += q
            rec["min_q16"][c] = min(rec["min_q16"][c], q)
    return rec


def cli_lines(rec, srec, bpp):
    """the two lines `pngloss --visible --distortion --ssim` prints for a written file"""
    mask = D.PSNR_MASK_OF_BPP[bpp]
    if rec["changed_pixels"] == 0:
        first = "  distortion (visible): none, %d visible pixels" % rec["pixels"]
    else:
        largest = max(rec["max_abs"][c] for c in range(4) if mask >> c & 1)
        first = "  distortion (visible): PSNR %.2f dB, %d of %d visible pixels changed, largest channel error %d" % (
            D.py_psnr_db(rec, mask), rec["changed_pixels"], rec["pixels"], largest)
    if srec["windows"] == 0:
        return first, "  ssim (visible): not measured (no 8x8 window with a visible pixel)"
    worst = min(srec["min_q16"][c] for c in range(4) if mask >> c & 1)
    return first, "  ssim (visible): mean %.4f, worst window %.4f, %d windows with visible pixels" % (S.py_mean(srec, mask), worst / 65536.0, srec["windows"])


# ---- the pairs of the stand-alone measurement ----

def _holes(rng, a, b):
    """a rectangle invisible in both images (with colour left in it), and alphas of 0, 3 and 255 sprinkled over both independently"""
    h, w = a.shape[:2]
    if not a.size:
        return
    for img in (a, b):
        pick = rng.random((h, w))
        img[..., 3][pick < 0.15] = 0
        img[..., 3][(pick >= 0.15) & (pick < 0.25)] = 3
        img[..., 3][pick > 0.8] = 255
    a[: (h + 1) // 2, : (w + 1) // 2, 3] = 0
    b[: (h + 1) // 2, : (w + 1) // 2, 3] = 0


@functools.lru_cache(maxsize=None)
def distort_pairs():
    """the mixed shapes of tests/util_distort.py with transparency put into them: [(a, b)] read-only"""
    rng = np.random.default_rng(23)
    out = []
    for a, b in D.mixed_pairs():
        a, b = a.copy(), b.copy()
        _holes(rng, a, b)
        a.setflags(write=False); b.setflags(write=False)
        out.append((a, b))
    return out


def _pair(rng, w, h):
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    return a, b


@functools.lru_cache(maxsize=None)
def ssim_pairs():
    """name -> (a, b), read-only: one window; no window; 16 x 8 with columns 0-7 invisible in both images (windows at x = 0, 4, 8: the first is dropped);
    133 x 37, whose 32 x 8 windows fill one tile to the brim, on the word-by-word path (odd width); 136 x 40, 33 x 9 windows and so two tiles each way,
    on the 16-byte path; 137 x 41, the same two tiles each way word by word"""
    rng = np.random.default_rng(29)
    out = {}
    a, b = _pair(rng, 8, 8)
    a[..., 3][a[..., 3] < 64] = 0
    out["8x8"] = (a, b)
    out["7x64"] = _pair(rng, 7, 64)
    a, b = _pair(rng, 16, 8)
    a[..., 3] |= 1; b[..., 3] |= 1
    a[:, :8, 3] = 0; b[:, :8, 3] = 0
    out["16x8_left_invisible"] = (a, b)
    for w, h in ((133, 37), (136, 40), (137, 41)):
        a, b = _pair(rng, w, h)
        _holes(rng, a, b)
        a[:, w - 20:, 3] = 0; b[:, w - 20:, 3] = 0      # and a band of whole windows without a visible pixel at the right edge
        out["%dx%d" % (w, h)] = (a, b)
    for a, b in out.values():
        a.setflags(write=False); b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_pairs():
    """name -> (a, b), read-only: invisible in both images (colour differs: nothing to measure); alpha 0 -> 3 and 3 -> 0 (visible in one image only);
    fully opaque (visible mode = all-pixel mode)"""
    rng = np.random.default_rng(31)
    out = {}
    a, b = _pair(rng, 24, 16)
    a[..., 3] = 0; b[..., 3] = 0
    out["invisible"] = (a, b)
    a, b = _pair(rng, 24, 16)
    a[..., 3] = 0; b[..., 3] = 0
    a[:8, :, 3] = 0; b[:8, :, 3] = 3                    # 0 -> 3
    a[8:, :12, 3] = 3; b[8:, :12, 3] = 0                # 3 -> 0; the rest stays invisible in both
    out["alpha_0_3"] = (a, b)
    a, b = _pair(rng, 40, 24)
    a[..., 3] = 255; b[..., 3] = 255
    out["opaque"] = (a, b)
    for a, b in out.values():
        a.setflags(write=False); b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def trip_pairs():
    """[(name, a, b)], read-only: the pairs of S.trip_pairs() that take a workgroup of pl_ssim past its first tile -- the noise pairs with holes and a
    band of invisible windows at the right edge -- and a 300 x 77 pair invisible in both images (tiles to visit, no window to count)"""
    rng = np.random.default_rng(47)
    out = []
    for name, a, b in S.trip_pairs():
        if name.split("_")[1] in ("noise", "near"):
            a, b = a.copy(), b.copy()
            _holes(rng, a, b)
            a[:, a.shape[1] - 20:, 3] = 0; b[:, b.shape[1] - 20:, 3] = 0
        out.append((name, a, b))
    a, b = (x.copy() for x in S.contents(300, 77, seed=6)["noise"])
    a[..., 3] = 0; b[..., 3] = 0
    out.append(("300x77_invisible", a, b))
    for _, a, b in out:
        a.setflags(write=False); b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def trip_expected():
    """(distortion record, SSIM record) of trip_pairs() in visible mode; the two uniform pairs by S.uniform_record's closed form (every window of
    theirs holds a visible pixel; tests/test_visible_host.py checks it against py_ssim on the whole pair)"""
    return [(np_distortion(a, b), S.uniform_record(a, b, py_ssim) if name in ("1036x1028_checkerboard_inverse", "1032x1032_equal") else py_ssim(a, b))
            for name, a, b in trip_pairs()]


#: pairs of a call that a single launch cannot take (D.MAX_IMAGES = 65535 images a launch): pair i is split_pool()[i % 7]
SPLIT_N = 65540


@functools.lru_cache(maxsize=None)
def split_pool():
    """[(name, a, b)], read-only: seven small pairs of seven different distortion records -- 1x1, 3x1, 8x8 (one window), 12x12 (four),
    13x9 (two), 16x8 with holes, and one without pixels"""
    rng = np.random.default_rng(53)
    out = []
    for w, h in ((1, 1), (3, 1), (8, 8), (12, 12), (13, 9), (16, 8), (0, 0)):
        a, b = _pair(rng, w, h)
        if a.size:
            a[..., 3] |= 1                                  # visible: the all-pixel and the visible pixel counts agree but for the holes
        if (w, h) == (16, 8):
            _holes(rng, a, b)
        a.setflags(write=False); b.setflags(write=False)
        out.append(("%dx%d" % (w, h), a, b))
    return out


# ---- the images of the batch and search tests, and the CPU oracle on them ----

BATCH_SHAPES = [(64, 48), (96, 64), (40, 8)]


@functools.lru_cache(maxsize=None)
def batch_images():
    """three RGBA images: a smooth colour field with noise on it, alpha an opaque disc with a soft rim, the rest (most of the image) transparent and of
    a single colour, as the transparent areas of real files are; read-only"""
    rng = np.random.default_rng(37)
    out = []
    for w, h in BATCH_SHAPES:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.zeros((h, w, 4), np.float64)
        for c in range(3):
            img[..., c] = 128 + 90 * np.sin(xx / (5.0 + 2 * c) + c) * np.cos(yy / (7.0 - c)) + rng.normal(0, 14, (h, w))
        r = np.hypot((xx - w * 0.35) / (w * 0.33), (yy - h * 0.5) / (h * 0.48))
        img[..., 3] = np.clip((1.0 - r) * 6.0, 0, 1) * 255
        img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        img[img[..., 3] == 0] = (255, 255, 255, 0)
        img.setflags(write=False)
        out.append(img)
    return out


@functools.lru_cache(maxsize=None)
def oracle_probe(index, strength):
    """batch_images()[index] through the CPU oracle at `strength`, bleed 2: (original, pixels, row filters, bytes per pixel, all-pixel distortion record,
    all-pixel SSIM record, visible distortion record, visible SSIM record), from the oracle and numpy alone; cached and read-only"""
    img = batch_images()[index]
    out, filt = U.run_port(img, strength, T.BLEED)
    out.setflags(write=False); filt.setflags(write=False)
    return img, out, filt, T.bpp_of(out), D.np_distortion(img, out), S.py_ssim(img, out), np_distortion(img, out), py_ssim(img, out)


def oracle_search(index, m, min_psnr_db, min_ssim, visible):
    """the halving rule of the target search replayed on the CPU oracle, accepting on visible records or on all-pixel ones: (chosen, probe sequence)"""
    def accepted(s):
        _, _, _, bpp, rec, srec, vrec, vsrec = oracle_probe(index, s)
        return S.py_accept2(min_psnr_db, 0, min_ssim, vrec if visible else rec, vsrec if visible else srec, 0, bpp)

    return T.py_search(m, accepted)


#: the search of the tests: strengths up to SEARCH_M, both floors set.  tests/test_visible_host.py checks on the CPU oracle that at least one of the
#: three images ends at another strength under "visible" than under "all".
SEARCH_M, SEARCH_PSNR, SEARCH_SSIM = 40, 30.0, 0.97


# ---- the CPU harness ----

def build_visible_host(tmp_path):
    """tests/c/visible_host.cpp with -fsanitize=address,undefined (as D.build_distort_host builds its harness); returns the executable"""
    exe = str(tmp_path / "visible_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "visible_host.cpp")], check=True, capture_output=True)
    return exe


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def run_pm(exe):
    """pm of the pixel (c, c, c, A) from the C code, as a (256, 256) uint32 array indexed [A, c]"""
    lines = _run(exe, ["pm"])
    assert len(lines) == 65536
    return np.array([int(x, 16) for x in lines], np.uint32).reshape(256, 256)


def run_visible_host(exe, tmp_path, cases):
    """cases: (kind, a, b, a_offset, b_offset, nthreads) with kind "distort" | "ssim" and a, b (H, W, 4) uint8.  Returns one record dict per case;
    fails on any sanitizer report."""
    path = str(tmp_path / "visible_cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint64).tobytes())
        for kind, a, b, oa, ob, nt in cases:
            fh.write(np.array([{"distort": 0, "ssim": 1}[kind], a.shape[1], a.shape[0], oa, ob, nt], np.uint64).tobytes())
            fh.write(np.ascontiguousarray(a).tobytes())
            fh.write(np.ascontiguousarray(b).tobytes())
    lines = _run(exe, [path])
    assert len(lines) == len(cases)
    recs = []
    for (kind, *_), line in zip(cases, lines):
        v = [int(x) for x in line.split()]
        recs.append(dict(pixels=v[0], changed_pixels=v[1], sq_err=v[2:6], max_abs=v[6:10]) if kind == "distort"
                    else dict(windows=v[0], sum_q16=v[1:5], min_q16=v[5:9], reserved=v[9]))
    return recs

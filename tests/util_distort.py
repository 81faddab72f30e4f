"""Helpers of the distortion tests (tests/test_distort_host.py, tests/test_keep_layout_host.py, tests/test_gpu_distort.py): the numpy reference every
record is compared with, the shape list both the CPU harness and the GPU tests run, and the builders of the two CPU harnesses."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import util as U

#: (width, height) of the mixed batch: the vector tail (n % 4 = 1, 3), images smaller than a wave, more than one workgroup, and one without pixels
MIXED_SHAPES = [(1, 1), (3, 1), (63, 1), (65, 3), (257, 5), (1024, 7), (0, 0)]
PSNR_MASK_OF_BPP = {1: 0x2, 2: 0xA, 3: 0x7, 4: 0xF}


def np_distortion(a, b):
    """the record of two (H, W, 4) uint8 arrays (b against a), from numpy alone: int64 sums, np.abs().max(), a word compare"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape[-1] == 4
    d = b.astype(np.int64).reshape(-1, 4) - a.astype(np.int64).reshape(-1, 4)
    n = d.shape[0]
    changed = int((a.reshape(-1).view(np.uint32) != b.reshape(-1).view(np.uint32)).sum()) if n else 0
    return dict(pixels=n, changed_pixels=changed, sq_err=[int((d[:, c] ** 2).sum()) for c in range(4)],
                max_abs=[int(np.abs(d[:, c]).max()) if n else 0 for c in range(4)])


def py_psnr_db(rec, mask):
    """pngloss_hip_psnr_db's formula in Python"""
    if rec["pixels"] == 0 or mask == 0 or mask > 0xF:
        return math.nan
    chans = [c for c in range(4) if mask >> c & 1]
    s = sum(rec["sq_err"][c] for c in chans)
    return math.inf if s == 0 else 10.0 * math.log10(255.0 * 255.0 * float(rec["pixels"]) * float(len(chans)) / float(s))


def cli_line(rec, bpp):
    """the line `pngloss --distortion` prints for a written file"""
    if rec["changed_pixels"] == 0:
        return "  distortion: none (lossless)"
    mask = PSNR_MASK_OF_BPP[bpp]
    largest = max(rec["max_abs"][c] for c in range(4) if mask >> c & 1)
    return "  distortion: PSNR %.2f dB, %d of %d pixels changed, largest channel error %d" % (py_psnr_db(rec, mask), rec["changed_pixels"], rec["pixels"], largest)


def mixed_pairs(seed=11):
    """the pairs of MIXED_SHAPES: b random for every other pair, else a with about 1 % of its bytes changed"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (w, h) in enumerate(MIXED_SHAPES):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if k % 2 == 0:
            b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        else:
            b = a.copy()
            hit = rng.random(b.shape) < 0.01
            if b.size and not hit.any():
                hit.reshape(-1)[int(rng.integers(0, b.size))] = True
            b[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
        out.append((a, b))
    return out


def build_distort_host(tmp_path):
    """tests/c/distort_host.cpp with -fsanitize=address,undefined; returns the executable"""
    exe = str(tmp_path / "distort_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "distort_host.cpp")], check=True, capture_output=True)
    return exe


def run_distort_host(exe, tmp_path, cases):
    """cases: (a, b, a_offset, b_offset, nthreads) with a, b (H, W, 4) uint8.  Returns one record dict per case; fails on any sanitizer report."""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint64).tobytes())
        for a, b, oa, ob, nt in cases:
            fh.write(np.array([a.size // 4, oa, ob, nt], np.uint64).tobytes())
            fh.write(np.ascontiguousarray(a).tobytes())
            fh.write(np.ascontiguousarray(b).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    recs = []
    for line in r.stdout.splitlines():
        v = [int(x) for x in line.split()]
        recs.append(dict(pixels=v[0], changed_pixels=v[1], sq_err=v[2:6], max_abs=v[6:10]))
    assert len(recs) == len(cases)
    return recs


# ---- the launch shape of pl_keep and pl_distort (pl_distort_core.h: pld_grid_blocks, PLD_MAX_IMAGES, PLD_THREADS, PLD_FLUSH_PIXELS), restated ----

#: a launch takes at most this many images; lanes per workgroup; a lane empties its 32-bit sums once it has taken this many pixels
MAX_IMAGES, THREADS, FLUSH_PIXELS = 65535, 256, 16384


def grid_blocks(n, max_pixels):
    """workgroups per image of a launch of n images whose largest has max_pixels pixels: min(ceil(max_pixels / 4096), max(8, ceil(2048 / n))), at
    least 1"""
    assert n >= 1
    return max(1, min(-(-max_pixels // (THREADS * 16)), max(8, -(-2048 // n))))


#: the rule at the points the CPU test pins, written out: {max_pixels: blocks for n = GRID_N}
GRID_N = [1, 5, 59, 255, 256, 257, 300, 65535]
GRID_POINTS = {
    0: [1, 1, 1, 1, 1, 1, 1, 1],
    1: [1, 1, 1, 1, 1, 1, 1, 1],
    4096: [1, 1, 1, 1, 1, 1, 1, 1],
    4097: [2, 2, 2, 2, 2, 2, 2, 2],
    33587200: [2048, 410, 35, 9, 8, 8, 8, 8],
}


def lane_pixels(n, max_pixels, pixels, vector=True):
    """the most pixels one lane takes of an image of `pixels` in a launch of n images whose largest has max_pixels: quads (16-byte path) or words at a
    stride of every lane of the image's workgroups"""
    lanes = grid_blocks(n, max_pixels) * THREADS
    return 4 * -(-(pixels // 4) // lanes) if vector else -(-pixels // lanes)


def run_distort_grid(exe, points):
    """points: (n, max_pixels) each.  Returns (PLD_MAX_IMAGES, PLD_THREADS, [pld_grid_blocks(n, max_pixels)]) from the C code"""
    r = subprocess.run([exe, "grid"] + [str(v) for p in points for v in p], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(points) + 1
    return int(lines[0].split()[0]), int(lines[0].split()[1]), [int(x) for x in lines[1:]]


# ---- many records at once: the ctypes array a compare call filled, seen through numpy ----

#: PlDistortRecord / pngloss_hip_distortion as a numpy record
RECORD_DTYPE = np.dtype([("pixels", "<u8"), ("changed_pixels", "<u8"), ("sq_err", "<u8", (4,)), ("max_abs", "<u4", (4,))])


def records_array(recs, dtype=RECORD_DTYPE):
    """the list of structures a compare call returned (items of ONE ctypes array) as a numpy array of records over the same memory"""
    assert dtype.itemsize == 64 == C.sizeof(type(recs[0]))
    return np.frombuffer(recs[0]._b_base_, dtype=dtype, count=len(recs))


def dicts_array(dicts, dtype=RECORD_DTYPE):
    """record dicts (np_distortion, py_ssim) as a numpy array of records"""
    out = np.zeros(len(dicts), dtype)
    for k, d in enumerate(dicts):
        for name in dtype.names:
            out[name][k] = d[name]
    return out


def differing(got, want):
    """indices at which two record arrays differ in any byte"""
    g, w = (np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1) for x in (got, want))
    return np.flatnonzero((g != w).any(axis=1))


_keep = None


def keep_layout_lib():
    """tests/c/keep_layout_host.cpp (pl_keep_layout of pngloss_amd/csrc/pl_layout.h behind a C ABI) built into a shared object (cached per process)"""
    global _keep
    if _keep is None:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="keep_layout_host_"), "libkeep_layout_host.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", so, os.path.join(U.ROOT, "tests", "c", "keep_layout_host.cpp")], check=True)
        lib = C.CDLL(so)
        lib.keep_layout_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.keep_layout_host.restype = None
        _keep = lib
    return _keep


def keep_layout(ws, hs, originals, job_bytes=32, record_bytes=64):
    n = len(ws)
    w, h = np.array(ws, np.uint32), np.array(hs, np.uint32)
    image, tables = np.zeros(max(n, 1), np.int64), np.zeros(3, np.int64)
    keep_layout_lib().keep_layout_host(w.ctypes.data, h.ctypes.data, n, int(originals), job_bytes, record_bytes, image.ctypes.data, tables.ctypes.data)
    return [int(x) for x in image[:n]], dict(jobs=int(tables[0]), records=int(tables[1]), total=int(tables[2]))

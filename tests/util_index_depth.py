"""Helpers of the bit-depth tests of the indexed-colour write side (tests/test_index_depth_host.py, tests/test_gpu_index_depth.py,
tests/test_gpu_index_depth_cli.py): the numpy restatement of include/pngloss_hip_index_depth.h -- min_depth, the packed scanlines, the rule that
names the stream to keep --, the inputs both the CPU and the GPU tests use, and the builder of the CPU harness.  Nothing here calls the code under
test for an expected value."""
import os
import subprocess
import zlib

import numpy as np

from tests import util as U
from tests import util_index as X

MODES = {"8": 0, "auto": 1, "min": 2}
PACK_LANES = 256               # pl_index_pack: a workgroup of 256 lanes strides over a packed row, one dword of it per lane ...
PACK_ROW_BLOCKS = 512          # ... and min(height, 512) workgroups an image stride over its rows
PACK_JOB_BYTES = 48            # sizeof(PlPackJob): pl_index.h pins it with a static_assert, tests/c/index_depth_host.cpp lays the table out with it


def trip_pixels(depth):
    """pixels one trip of a workgroup of pl_index_pack covers: 8192 / 4096 / 2048 at depth 1 / 2 / 4"""
    return PACK_LANES * 32 // depth


def min_depth(entries):
    if 1 <= entries <= 2:
        return 1
    if 3 <= entries <= 4:
        return 2
    if 5 <= entries <= 16:
        return 4
    return 8 if 17 <= entries <= 256 else 0


def pack_rows(rows, depth):
    """(H, W) uint8 palette indices -> (H, ceil(W * depth / 8)) uint8: pixel x in byte x * depth / 8 at the shift 8 - depth * (x % (8 / depth) + 1);
    the unused low bits of the last byte are 0"""
    assert depth in (1, 2, 4)
    rows = np.asarray(rows, np.uint8)
    h, w = rows.shape
    per = 8 // depth
    nbytes = (w * depth + 7) // 8
    padded = np.zeros((h, nbytes * per), np.uint16)
    padded[:, :w] = rows
    shifts = (8 - depth * (np.arange(per) + 1)).astype(np.uint16)
    return (padded.reshape(h, nbytes, per) << shifts).sum(axis=2).astype(np.uint8)


def unpack_rows(packed, width, depth):
    """the other way round: (H, bytes) uint8 -> (H, width) uint8 indices"""
    packed = np.asarray(packed, np.uint8)
    per = 8 // depth
    shifts = (8 - depth * (np.arange(per) + 1)).astype(np.uint8)
    idx = (packed[:, :, None] >> shifts) & ((1 << depth) - 1)
    return idx.reshape(packed.shape[0], -1)[:, :width].astype(np.uint8)


def scanlines(rows, depth):
    """the scanlines of (H, W) index rows at bit depth 8, 4, 2 or 1: per row the filter type byte 0 and the row's bytes"""
    body = np.asarray(rows, np.uint8) if depth == 8 else pack_rows(rows, depth)
    return b"".join(b"\0" + body[y].tobytes() for y in range(body.shape[0]))


def choose(mode, colors, T, I8, Ip, trns_entries):
    """(bit depth of the stream that is kept, 0 for truecolour; size of the indexed candidate compared with T): the smallest of the candidates the
    mode has -- T, I8 + overhead, Ip + overhead --, a tie to the earlier one.  colors: 0 or 257 for an image that is not eligible"""
    md = min_depth(colors)
    cands = [(T, 0, 0)]
    if md:
        ov = X.overhead(colors, trns_entries)
        if mode != "min" or md == 8:
            cands.append((I8 + ov, 1, 8))
        if mode != "8" and md < 8:
            cands.append((Ip + ov, 2, md))
    best = min(cands)                                   # by cost, then by order
    indexed = [c for c in cands if c[1]]
    return best[2], (min(indexed)[0] - X.overhead(colors, trns_entries) if indexed else 0)


def opaque_colours(n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(1 << 24, n, replace=False).astype(np.uint32) | np.uint32(0xFF000000))


def noise(colors, width, height, seed):
    """uniformly random pixels over `colors` opaque colours, every colour present"""
    rng = np.random.default_rng(seed)
    pal = opaque_colours(colors, seed + 1000)
    idx = rng.integers(0, colors, width * height)
    idx[:colors] = np.arange(colors)
    return X.from_words(pal[idx], width, height)


def noise_inputs():
    """name -> image: the inputs on which the packed stream must win (tests/test_index_depth_host.py records the condition with zlib level 9)"""
    return {"noise_2_64x64": noise(2, 64, 64, 5), "noise_4_64x64": noise(4, 64, 64, 6), "noise_16_256x256": noise(16, 256, 256, 7)}


def structured_inputs():
    """name -> image: horizontal runs of 16 colours, and vertical stripes of three colours with a period of 3 pixels"""
    rng = np.random.default_rng(11)
    pal = opaque_colours(16, 12)
    w, h = 96, 64
    words = np.empty(w * h, np.uint32)
    at = 0
    while at < w * h:
        n = int(rng.integers(5, 40))
        words[at:at + n] = pal[rng.integers(0, 16)]
        at += n
    words[:16] = pal
    runs = X.from_words(words, w, h)
    stripes = X.from_words(np.tile(pal[np.arange(w) % 3], h), w, h)
    assert X.restate(runs)["colors"] == 16 and X.restate(stripes)["colors"] == 3
    return {"runs_16_96x64": runs, "stripes_3_96x64": stripes}


def filtered_rgb_rows(img, filt):
    """the RGB scanlines of an opaque (H, W, 4) image with one filter type (0 none, 1 sub, 2 up) on every row"""
    rgb = np.ascontiguousarray(img[:, :, :3]).astype(np.int16)
    h, w = rgb.shape[:2]
    flat = rgb.reshape(h, w * 3)
    if filt == 1:
        out = flat.copy()
        out[:, 3:] -= flat[:, :-3]
    elif filt == 2:
        out = flat.copy()
        out[1:] -= flat[:-1]
    else:
        out = flat
    out = (out & 255).astype(np.uint8)
    return b"".join(bytes([filt]) + out[y].tobytes() for y in range(h))


def zlib9_sizes(img):
    """(T, I8, Ip, overhead, min_depth) of an opaque image with zlib level 9 on the CPU: T the best of filter 0 / 1 / 2 RGB rows"""
    r = X.restate(img)
    md = min_depth(r["entries"])
    T = min(len(zlib.compress(filtered_rgb_rows(img, f), 9)) for f in (0, 1, 2))
    I8 = len(zlib.compress(scanlines(r["rows"], 8), 9))
    Ip = len(zlib.compress(scanlines(r["rows"], md), 9))
    return T, I8, Ip, X.overhead(r["entries"], r["trns_entries"]), md


# ---- tests/c/index_depth_host.cpp: the pack body, the rule and the layout on the CPU, under the sanitizers ----

def build_index_depth_host(tmp_path):
    exe = str(tmp_path / "index_depth_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "index_depth_host.cpp")], check=True, capture_output=True)
    return exe


def run_harness(exe, args, stdin=""):
    """stdout of one run of the harness; fails on any sanitizer report"""
    r = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def run_pack(exe, tmp_path, cases):
    """cases: (depth, (H, W) uint8 index rows).  Returns per case (pitch8, pitch, (H, pitch) uint8 packed rows as the body of pl_index_pack leaves
    them in memory prefilled with 0xEE)."""
    path, out_path = str(tmp_path / "pack_cases.bin"), str(tmp_path / "pack_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for depth, rows in cases:
            fh.write(np.array([depth, rows.shape[1], rows.shape[0]], np.uint32).tobytes())
            fh.write(np.ascontiguousarray(rows, np.uint8).tobytes())
    run_harness(exe, ["pack", path, out_path])
    raw = np.fromfile(out_path, np.uint8)
    got, at = [], 0
    for depth, rows in cases:
        pitch8, pitch = (int(x) for x in raw[at:at + 8].view("<u4"))
        at += 8
        h = rows.shape[0]
        got.append((pitch8, pitch, raw[at:at + h * pitch].reshape(h, pitch).copy()))
        at += h * pitch
    assert at == raw.size
    return got


def png_file(width, height, depth, ctype, zstream, plte=None, trns=None):
    """a PNG file around a finished zlib stream: IHDR, PLTE and tRNS where given, one IDAT, IEND"""
    import struct

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, ctype, 0, 0, 0))
    if plte:
        out += chunk(b"PLTE", plte)
    if trns:
        out += chunk(b"tRNS", trns)
    return out + chunk(b"IDAT", zstream) + chunk(b"IEND", b"")


def pixels_of(scanline_bytes, width, height, depth, plte, trns):
    """the RGBA8 image a palette file's inflated scanlines stand for"""
    nbytes = width if depth == 8 else (width * depth + 7) // 8
    body = np.frombuffer(scanline_bytes, np.uint8).reshape(height, 1 + nbytes)
    assert not body[:, 0].any()                                            # filter type 0 on every row
    idx = body[:, 1:] if depth == 8 else unpack_rows(body[:, 1:], width, depth)
    pal = np.zeros((256, 4), np.uint8)
    pal[:, 3] = 255
    pal[: len(plte) // 3, :3] = np.frombuffer(plte, np.uint8).reshape(-1, 3)
    pal[: len(trns), 3] = np.frombuffer(trns, np.uint8)
    assert int(idx.max()) < len(plte) // 3
    return pal[idx]


def report_line(r):
    """the -v line of a file kept below 8 bits (the mirror of cli_report_index_depth); empty for any other file"""
    if not 1 <= r["bit_depth"] < 8:
        return ""
    if r["indexed8_bytes"]:
        return f"  index depth: {r['bit_depth']} bits, {r['packed_bytes']} bytes of packed image data against {r['indexed8_bytes']} bytes at 8 bits\n"
    return f"  index depth: {r['bit_depth']} bits, {r['packed_bytes']} bytes of packed image data (the 8-bit stream was not written)\n"

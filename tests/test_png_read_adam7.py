"""PNG READ side, Adam7-interlaced files: the seven passes of such a file are seven filtered images in one zlib stream; the device reader
unfilters each pass as an image of its own and scatters its pixels to their places (pl_pngread.hip, one job per non-empty pass).  Expected
outputs come from the REAL reference reader (rwpng_read_image24, /root/reference/src/rwpng.c:422, which reads interlaced files through
png_set_interlace_handling; tests/golden/make_png_read_adam7_golden.py): every colour type x bit depth x tRNS, every size up to 9 x 9, a
few large files and two suite files re-encoded interlaced.
  not gpu: the pass geometry of pl_pngread_core.h, the CPU de-interlacer built on it (tests/c/pngread_adam7_host.cpp), the command line
           tool's chunk walk + inflate (png_stream_reader.c)
  gpu:     the three device entry points, a mixed batch, a damaged pass, random scanlines, the command line tool's --gpu-read"""
import ctypes as C
import os
import re
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U

TABLE = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]     # x0, y0, dx, dy
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}

_a7 = None


def adam7_lib():
    """tests/c/pngread_adam7_host.cpp as a shared object"""
    global _a7
    if _a7 is None:
        so = os.path.join(tempfile.mkdtemp(prefix="pngread_adam7_"), "libpngread_adam7.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-o", so, os.path.join(U.ROOT, "tests", "c", "pngread_adam7_host.cpp")], check=True)
        lib = C.CDLL(so)
        lib.pngread_adam7_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32,
                                             C.c_char_p, C.c_uint32, C.c_void_p]
        lib.pngread_adam7_decode.restype = C.c_int
        lib.pngread_adam7_pass.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64 * 8)]
        lib.pngread_adam7_pass.restype = None
        lib.pngread_adam7_total.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64 * 7)]
        lib.pngread_adam7_total.restype = C.c_uint64
        _a7 = lib
    return _a7


def fixtures():
    """(name, png bytes, expected RGBA8 of the REAL reference reader) of tests/golden/png_read_adam7_cases.npz"""
    g = U.load_npz("png_read_adam7_cases.npz")
    return [(k[:-4], g[k].tobytes(), g[k[:-4] + "/rgba"]) for k in g.files if k.endswith("/png")]


def cpu_decode(scan, w, h, ctype, depth, interlace, plte=None, trns=None):
    out = np.zeros((h, w, 4), np.uint8)
    rc = adam7_lib().pngread_adam7_decode(scan, len(scan), w, h, ctype, depth, interlace, plte, len(plte) // 3 if plte else 0, trns,
                                          len(trns) if trns else 0, out.ctypes.data)
    return rc, out


def py_pass(p, w, h, ctype, depth):
    """the table of the PNG specification, stated once more in Python"""
    x0, y0, dx, dy = TABLE[p]
    pw = (w - x0 + dx - 1) // dx if w > x0 else 0
    ph = (h - y0 + dy - 1) // dy if h > y0 else 0
    rb = (pw * CHANNELS[ctype] * depth + 7) // 8
    return [x0, y0, dx, dy, pw, ph, rb, ph * (1 + rb) if pw and ph else 0]


def test_pass_geometry_matches_the_table():
    lib = adam7_lib()
    out, off = (C.c_uint64 * 8)(), (C.c_uint64 * 7)()
    sizes = [(w, h) for w in range(1, 41) for h in range(1, 41)] + [(1000000, 1), (1, 1000000), (999999, 77777), (268435455, 3), (65537, 65539)]
    for ctype, depth in [(6, 8), (0, 1), (0, 2), (3, 4), (2, 16), (4, 8)]:
        for w, h in sizes:
            want = [py_pass(p, w, h, ctype, depth) for p in range(7)]
            for p in range(7):
                lib.pngread_adam7_pass(p, w, h, ctype, depth, C.byref(out))
                assert list(out) == want[p], (ctype, depth, w, h, p)
            total = lib.pngread_adam7_total(w, h, ctype, depth, C.byref(off))
            assert total == sum(s[7] for s in want) and list(off) == [sum(s[7] for s in want[:p]) for p in range(7)], (ctype, depth, w, h)
    # every pixel of an image belongs to exactly one pass
    for w, h in [(1, 1), (9, 9), (17, 5), (40, 33)]:
        seen = np.zeros((h, w), np.int32)
        for p in range(7):
            x0, y0, dx, dy, pw, ph = py_pass(p, w, h, 6, 8)[:6]
            seen[y0:y0 + ph * dy:dy, x0:x0 + pw * dx:dx] += 1
        assert (seen == 1).all(), (w, h)


def test_source_structs_keep_their_layout():
    """`interlace` went into padding behind bit_depth: sizes and the other offsets stay; the positional forms of before still work"""
    assert C.sizeof(L.PngSource) == 64 and L.PngSource.interlace.offset == 18 and L.PngSource.palette.offset == 24 and L.PngSource.rgba.offset == 56
    assert C.sizeof(L.PngZSource) == 64 and L.PngZSource.interlace.offset == 26 and L.PngZSource.palette.offset == 32
    s = L.PngSource(b"xy", 3, 4, 2, 8, None, 0, None, 0, None)
    assert (s.width, s.height, s.color_type, s.bit_depth, s.interlace) == (3, 4, 2, 8, 0)
    assert L.PngSource(b"xy", 3, 4, 2, 8, None, 0, None, 0, None, interlace=1).interlace == 1
    z = L.PngZSource(b"xy", 2, 5, 6, 0, 16, None, 0, None, 0, interlace=1)
    assert (z.zbytes, z.width, z.height, z.bit_depth, z.interlace) == (2, 5, 6, 16, 1)


def test_fixture_set_covers_every_format_and_every_small_size():
    names = {n for n, _, _ in fixtures()}
    for ctype, depths in [(0, [1, 2, 4, 8, 16]), (2, [8, 16]), (3, [1, 2, 4, 8]), (4, [8, 16]), (6, [8, 16])]:
        for d in depths:
            for trns in (["plain", "trns"] if ctype in (0, 2, 3) else ["plain"]):
                for size in ("37x19", "130x70"):
                    assert "i_t%d_d%d_%s_%s" % (ctype, d, trns, size) in names
    for w in range(1, 10):
        for h in range(1, 10):
            assert "i_t6_d8_plain_%dx%d" % (w, h) in names and "i_t0_d1_plain_%dx%d" % (w, h) in names
    for p in fixtures():
        assert L.parse_png(p[1])["interlace"] == 1, p[0]


def test_cpu_deinterlacer_matches_the_reference_reader():
    n = 0
    for name, png, want in fixtures():
        p = L.parse_png(png)
        rc, out = cpu_decode(p["scanlines"], p["width"], p["height"], p["ctype"], p["depth"], 1, p["plte"], p["trns"])
        assert rc == 0 and np.array_equal(out, want), name
        n += 1
    assert n == 219


def test_fixtures_are_what_the_reference_reader_makes():
    if not os.path.exists(os.path.join(U.ROOT, "oracle", "_ref", "librwpng_ref.so")):
        pytest.skip("oracle/_ref/librwpng_ref.so is built where the reference tree exists")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_png_read_golden", os.path.join(U.GOLDEN, "make_png_read_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    read = mod.ref_reader()
    for name, png, want in fixtures():
        assert np.array_equal(read(png), want), name


class StreamSource(C.Structure):
    """png_stream_source of pngloss_amd/cli/png_stream_reader.h"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("color_type", C.c_uint8), ("bit_depth", C.c_uint8), ("interlace", C.c_uint8),
                ("scanlines", C.c_void_p), ("scanline_bytes", C.c_size_t), ("palette", C.c_ubyte * 768), ("palette_entries", C.c_uint32),
                ("trns", C.c_ubyte * 256), ("trns_bytes", C.c_uint32), ("has_trns", C.c_bool), ("has_srgb", C.c_bool), ("has_gama", C.c_bool),
                ("gamma", C.c_double), ("file_size", C.c_size_t)]


def test_cli_stream_reader_takes_interlaced_files(tmp_path):
    """The command line tool's host half of --gpu-read (png_stream_reader.c, compiled here with gcc and zlib) takes every interlaced fixture and
    inflates exactly the Adam7 total; an unknown interlace method still goes to libpng (false)."""
    so = str(tmp_path / "libstream_reader.so")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-w", "-shared", "-fPIC", "-o", so, os.path.join(U.ROOT, "pngloss_amd", "cli", "png_stream_reader.c"), "-lz"],
                   check=True)
    lib = C.CDLL(so)
    lib.png_stream_read.argtypes = [C.c_char_p, C.POINTER(StreamSource)]
    lib.png_stream_read.restype = C.c_bool
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    total = adam7_lib().pngread_adam7_total
    off = (C.c_uint64 * 7)()
    path = str(tmp_path / "f.png")
    for name, png, _ in fixtures():
        open(path, "wb").write(png)
        s = StreamSource()
        assert lib.png_stream_read(path.encode(), C.byref(s)), name
        p = L.parse_png(png)
        want = total(p["width"], p["height"], p["ctype"], p["depth"], C.byref(off))
        assert s.interlace == 1 and s.scanline_bytes == want == len(p["scanlines"]), name
        assert C.string_at(s.scanlines, s.scanline_bytes) == p["scanlines"], name
        libc.free(s.scanlines)
    # interlace method 2 (no such method): not this reader's
    png = bytearray(fixtures()[0][1])
    png[8 + 8 + 12] = 2
    crc = zlib.crc32(bytes(png[12:12 + 4 + 13])) & 0xffffffff
    png[12 + 4 + 13:12 + 4 + 13 + 4] = crc.to_bytes(4, "big")
    open(path, "wb").write(bytes(png))
    s = StreamSource()
    assert not lib.png_stream_read(path.encode(), C.byref(s))


# ---- on the device ---------------------------------------------------------------------------------------------------------------

def _device_bytes(ptr, nbytes):
    path = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l][0]
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _frame(f):
    ptr, w, h = f
    return _device_bytes(ptr, w * h * 4).reshape(h, w, 4)


@pytest.mark.gpu
def test_device_reader_decodes_interlaced_files():
    fx = fixtures()
    ctx = P.HipContext()
    outs = ctx.png_decode([png for _, png, _ in fx])
    for (name, _, want), out in zip(fx, outs):
        assert np.array_equal(out, want), (name, np.argwhere((out != want).any(axis=2))[:3].tolist())
    for name, png, want in fx[::23] + fx[-5:]:
        assert np.array_equal(ctx.png_decode([png])[0], want), name
    ctx.close()


@pytest.mark.gpu
def test_device_reader_mixed_batch():
    """the 78 non-interlaced fixtures of tests/test_png_read.py and the interlaced ones, interleaved in one batch"""
    plain, inter = U.png_read_fixtures(), fixtures()
    assert len(plain) == 78
    mixed = []
    for k in range(max(len(plain), len(inter))):
        mixed += ([plain[k]] if k < len(plain) else []) + ([inter[k]] if k < len(inter) else [])
    ctx = P.HipContext()
    outs, st, rc = ctx.png_decode_status([png for _, png, _ in mixed])
    assert rc == 0 and not any(st)
    for (name, _, want), out in zip(mixed, outs):
        assert np.array_equal(out, want), name
    ctx.close()


@pytest.mark.gpu
def test_device_frames_of_interlaced_files_feed_the_optimiser():
    """pngloss_hip_png_decode_batch_device (scanlines up) and _device_z (the inflate on the device too) give the reference reader's frames;
    a few of them go straight into the optimiser of the same context"""
    import torch
    fx = fixtures()
    ctx = P.HipContext()
    frames, st = ctx.png_decode_device([png for _, png, _ in fx])
    assert not any(st)
    for (name, _, want), f in zip(fx, frames):
        assert f[0] % 256 == 0 and np.array_equal(_frame(f), want), name
    pick = [i for i, f in enumerate(fx) if f[0] in ("i_suite_rose", "i_suite_tux", "i_t6_d8_plain_130x70", "i_t2_d8_trns_1030x66", "i_t0_d1_plain_9x7")]
    assert len(pick) == 5
    filt = [torch.zeros(fx[i][2].shape[0], dtype=torch.uint8, device="cuda") for i in pick]
    res = ctx.run([(frames[i][0], f.data_ptr(), frames[i][1], frames[i][2]) for i, f in zip(pick, filt)], 19, 2)
    torch.cuda.synchronize()
    for i, f, r in zip(pick, filt, res):
        want, wf = U.run_port(fx[i][2], 19, 2)
        assert r["status"] == 0 and np.array_equal(_frame(frames[i]), want) and np.array_equal(f.cpu().numpy(), wf), fx[i][0]
    frames, st, rc = ctx.png_decode_device_z([png for _, png, _ in fx])
    assert rc == 0 and not any(st)
    for (name, _, want), f in zip(fx, frames):
        assert np.array_equal(_frame(f), want), name
    filt = [torch.zeros(fx[i][2].shape[0], dtype=torch.uint8, device="cuda") for i in pick]
    res = ctx.run([(frames[i][0], f.data_ptr(), frames[i][1], frames[i][2]) for i, f in zip(pick, filt)], 19, 2)
    torch.cuda.synchronize()
    for i, f, r in zip(pick, filt, res):
        want, wf = U.run_port(fx[i][2], 19, 2)
        assert r["status"] == 0 and np.array_equal(_frame(frames[i]), want) and np.array_equal(f.cpu().numpy(), wf), fx[i][0]
    ctx.close()


def _host_status(ctx, srcs):
    lib = P.hip_lib()
    arr = (L.PngSource * len(srcs))(*srcs)
    st = (C.c_int * len(srcs))()
    rc = lib.pngloss_hip_png_decode_batch_host_status(ctx._ctx, arr, len(srcs), st)
    return rc, list(st)


def _source(p, scan, out, interlace):
    return L.PngSource(scan, p["width"], p["height"], p["ctype"], p["depth"], p["plte"], len(p["plte"]) // 3 if p["plte"] else 0,
                       p["trns"], len(p["trns"]) if p["trns"] else 0, out.ctypes.data, interlace=interlace)


@pytest.mark.gpu
def test_device_reader_damaged_pass_fails_its_file_alone():
    """filter type 7 in the second row of pass 3 of one file: that file gets status 25, the others of the batch are decoded"""
    fx = [f for f in fixtures() if f[0] in ("i_t6_d8_plain_37x19", "i_t2_d16_trns_130x70", "i_t3_d4_plain_37x19", "i_t0_d1_plain_9x9")]
    assert len(fx) == 4
    parsed = [L.parse_png(f[1]) for f in fx]
    p = parsed[1]
    off = (C.c_uint64 * 7)()
    adam7_lib().pngread_adam7_total(p["width"], p["height"], p["ctype"], p["depth"], C.byref(off))
    x0, y0, dx, dy, pw, ph, rb, nb = py_pass(3, p["width"], p["height"], p["ctype"], p["depth"])
    assert ph >= 2
    bad = bytearray(p["scanlines"])
    assert bad[off[3] + 1 + rb] <= 4
    bad[off[3] + 1 + rb] = 7
    outs = [np.zeros((q["height"], q["width"], 4), np.uint8) for q in parsed]
    ctx = P.HipContext()
    rc, st = _host_status(ctx, [_source(q, bytes(bad) if i == 1 else q["scanlines"], o, 1) for i, (q, o) in enumerate(zip(parsed, outs))])
    assert rc == 25 and st == [0, 25, 0, 0]
    for i in (0, 2, 3):
        assert np.array_equal(outs[i], fx[i][2]), fx[i][0]
    ctx.close()


@pytest.mark.gpu
def test_device_reader_rejects_unknown_interlace_methods():
    name, png, _ = fixtures()[0]
    p = L.parse_png(png)
    out = np.zeros((p["height"], p["width"], 4), np.uint8)
    ctx = P.HipContext()
    rc, st = _host_status(ctx, [_source(p, p["scanlines"], out, 2)])
    assert rc == 4 and st == [4]
    lib = P.hip_lib()
    z = p["zstream"]
    zs = (L.PngZSource * 1)(L.PngZSource(z, len(z), p["width"], p["height"], p["ctype"], p["depth"], p["plte"], len(p["plte"]) // 3 if p["plte"] else 0,
                                         p["trns"], len(p["trns"]) if p["trns"] else 0, interlace=2))
    ptrs, st = (C.c_void_p * 1)(), (C.c_int * 1)()
    assert lib.pngloss_hip_png_decode_batch_device_z(ctx._ctx, zs, 1, ptrs, st, None) == 4 and st[0] == 4 and not ptrs[0]
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ctype,depth", [(4099, 300, 2, 8), (2000, 700, 6, 8), (5000, 129, 3, 4), (7, 1000, 2, 16), (1, 1, 6, 8),
                                             (1500, 333, 0, 16), (3001, 77, 0, 1)])
def test_device_reader_interlaced_many_bands_and_blocks(w, h, ctype, depth):
    """random pass scanlines with random filter types (mostly average and paeth), sized so that passes are many bands of 64 rows and many
    960-byte blocks, against the CPU de-interlacer (pinned to the reference reader by the fixtures above)"""
    rng = np.random.default_rng(w * 7 + h)
    parts = []
    for p in range(7):
        _, _, _, _, pw, ph, rb, nb = py_pass(p, w, h, ctype, depth)
        if nb:
            rows = rng.integers(0, 256, (ph, 1 + rb), dtype=np.uint8)
            rows[:, 0] = rng.choice([0, 1, 2, 3, 4, 3, 4, 4], ph)
            parts.append(rows.tobytes())
    scan = b"".join(parts)
    plte = bytes(rng.integers(0, 256, 3 * 16, dtype=np.uint8)) if ctype == 3 else None
    trns = bytes(rng.integers(0, 256, 9, dtype=np.uint8)) if ctype == 3 else None
    rc, want = cpu_decode(scan, w, h, ctype, depth, 1, plte, trns)
    assert rc == 0
    got = np.zeros((h, w, 4), np.uint8)
    p = dict(width=w, height=h, ctype=ctype, depth=depth, plte=plte, trns=trns)
    ctx = P.HipContext()
    rc, st = _host_status(ctx, [_source(p, scan, got, 1)])
    assert rc == 0 and st == [0]
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:3].tolist()
    ctx.close()


OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
REF_CLI = os.path.join(U.ROOT, "oracle", "_ref", "pngloss_ref_cli")
needs_our_cli = pytest.mark.skipif(not (os.path.exists(OUR_CLI) and os.path.exists(REF_CLI)),
                                   reason="pngloss_amd/cli/pngloss or the reference CLI build is missing")


@pytest.mark.gpu
@needs_our_cli
def test_batch_cli_gpu_read_takes_interlaced_files(tmp_path):
    """--gpu-read on interlaced files: every one of them is decoded on the device (the read side's file count, PNGLOSS_HIP_DEBUG_SEAM), and the
    outputs are byte for byte what the tool writes without the option (libpng reading the files)"""
    fx = [f for f in fixtures() if "37x19" in f[0] or f[0].startswith("i_suite_") or f[0].endswith("_5x3") or f[0].endswith("_1x1")]
    a_dir, b_dir = tmp_path / "libpng", tmp_path / "gpu"
    a_dir.mkdir(); b_dir.mkdir()
    for name, png, _ in fx:
        for d in (a_dir, b_dir):
            (d / f"{name}.png").write_bytes(png)
    names = [f[0] for f in fx]
    env = dict(os.environ, PNGLOSS_HIP_DEBUG_SEAM="1")
    ra = subprocess.run([OUR_CLI, "-s", "19", "-b", "2"] + [str(a_dir / f"{n}.png") for n in names], capture_output=True, text=True, timeout=600)
    rb = subprocess.run([OUR_CLI, "--gpu-read", "-s", "19", "-b", "2"] + [str(b_dir / f"{n}.png") for n in names], capture_output=True, text=True,
                        timeout=600, env=env)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr[-600:], rb.stderr[-600:])
    counts = [int(c) for c in re.findall(r"read side: (\d+) files", rb.stderr)]
    assert sum(counts) == len(names), (counts, rb.stderr[-600:])
    for n in names:
        assert (a_dir / f"{n}-loss.png").read_bytes() == (b_dir / f"{n}-loss.png").read_bytes(), n

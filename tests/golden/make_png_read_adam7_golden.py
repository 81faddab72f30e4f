"""Generates the fixtures of the PNG READ side for Adam7-interlaced files, in the build container only:

  png_read_adam7_cases.npz   "<case>/png"   the bytes of an interlaced PNG file written by the little encoder below: the image split into
                                            its seven passes (PNG specification section 8.2), each filtered on its own with a random filter
                                            type 0..4 on every pass row, the zlib stream split over several IDAT chunks
                             "<case>/rgba"  what the REAL reference reader makes of it: rwpng_read_image24 (/root/reference/src/rwpng.c:422,
                                            which reads interlaced files through png_set_interlace_handling) through oracle/_ref/librwpng_ref.so

Cases: every colour type x bit depth x tRNS at 37x19 and 130x70; every size from 1x1 to 9x9 at RGBA8 and at gray 1-bit (every pattern
of empty passes and of sub-byte padding); 1030x66 RGB8 with tRNS, 300x520 RGBA8, 5000x9 palette 4-bit (many blocks / many bands in a
pass); two of the reference's suite files re-encoded interlaced.  The larger images are tiles with a little noise, to keep the file small.

usage: python tests/golden/make_png_read_adam7_golden.py   (after `make -C oracle ref`)"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_png_read_golden import chunk, filter_rows, paeth, ref_reader  # noqa: E402

PASSES = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]    # x0, y0, dx, dy
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def pack_rows(samples, depth):
    """(h, w, channels) samples at their own depth -> (h, rowbytes) uint8 scanlines without filter bytes (padding bits zero)."""
    h, w, c = samples.shape
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, w * c * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * c)
    bits = np.unpackbits(samples.reshape(h, w * c, 1).astype(np.uint8), axis=2)[:, :, 8 - depth:].reshape(h, w * c * depth)
    return np.packbits(bits, axis=1)


def unfilter(scan, h, rowbytes, bpp):
    """inverse of filter_rows: filtered stream -> (h, rowbytes) raw scanlines"""
    out = np.zeros((h, rowbytes), np.uint8)
    prev = np.zeros(rowbytes, np.int32)
    for y in range(h):
        row = scan[y * (rowbytes + 1):(y + 1) * (rowbytes + 1)]
        ft, f = row[0], np.frombuffer(row[1:], np.uint8).astype(np.int32)
        cur = np.zeros(rowbytes, np.int32)
        if ft in (0, 2):
            cur = (f + (prev if ft == 2 else 0)) & 255
        else:
            for i in range(rowbytes):
                a = cur[i - bpp] if i >= bpp else 0
                c = prev[i - bpp] if i >= bpp else 0
                pred = a if ft == 1 else ((a + prev[i]) >> 1 if ft == 3 else paeth(a, prev[i], c))
                cur[i] = (f[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out


def encode(samples, ctype, depth, extra, rng):
    """interlaced PNG of the (H, W, channels) samples; extra: PLTE / tRNS chunks"""
    h, w, c = samples.shape
    bpp = max(1, c * depth // 8)
    data = b""
    for x0, y0, dx, dy in PASSES:
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            data += filter_rows(pack_rows(sub, depth), bpp, rng)
    stream = zlib.compress(data, 9)
    cut = max(1, len(stream) // 3)
    idat = b"".join(chunk(b"IDAT", stream[i:i + cut]) for i in range(0, len(stream), cut))
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + extra + idat + chunk(b"IEND", b"")


def make_case(w, h, ctype, depth, trns, rng, smooth):
    c = CHANNELS[ctype]
    top = (1 << depth) - 1
    if smooth:
        # tiles of 13 x 3 pixels in six levels with a little noise: every filter still sees varied bytes, but zlib packs the file and the RGBA8 well
        tiles = (rng.integers(0, 6, ((h + 2) // 3, (w + 12) // 13, c)) * max(1, top // 5)) & top
        s = np.repeat(np.repeat(tiles, 3, axis=0), 13, axis=1)[:h, :w]
        s = np.where(rng.random((h, w, c)) < 0.005, rng.integers(0, top + 1, (h, w, c)), s)
    else:
        s = rng.integers(0, top + 1, (h, w, c))
    s = s.astype(np.int64)
    extra = b""
    if ctype == 3:
        n = 1 << depth
        extra += chunk(b"PLTE", rng.integers(0, 256, (n, 3), dtype=np.uint8).tobytes())
        if trns:
            extra += chunk(b"tRNS", rng.integers(0, 256, max(1, n // 2), dtype=np.uint8).tobytes())
    elif trns and ctype == 0:
        key = int(rng.integers(0, top + 1))
        s[rng.random((h, w)) < 0.2] = key                                   # the key really occurs
        extra += chunk(b"tRNS", struct.pack(">H", key))
    elif trns and ctype == 2:
        key = [int(v) for v in rng.integers(0, top + 1, 3)]
        s[rng.random((h, w)) < 0.25] = key
        extra += chunk(b"tRNS", struct.pack(">HHH", *key))
    return encode(s, ctype, depth, extra, rng)


def reencode_suite(png, rng):
    """a non-interlaced suite file -> the same image, interlaced (same colour type, depth, PLTE and tRNS)"""
    o, ihdr, extra, idat = 8, None, b"", []
    while o < len(png):
        n, tag = struct.unpack(">I4s", png[o:o + 8])
        body = png[o + 8:o + 8 + n]
        o += 12 + n
        if tag == b"IHDR": ihdr = body
        elif tag in (b"PLTE", b"tRNS"): extra += chunk(tag, body)
        elif tag == b"IDAT": idat.append(body)
    w, h, depth, ctype, _, _, il = struct.unpack(">IIBBBBB", ihdr)
    assert il == 0 and depth == 8
    c = CHANNELS[ctype]
    raw = unfilter(zlib.decompress(b"".join(idat)), h, w * c, c)
    return encode(raw.reshape(h, w, c).astype(np.int64), ctype, depth, extra, rng)


CASES = []
for ctype, depths in [(0, [1, 2, 4, 8, 16]), (2, [8, 16]), (3, [1, 2, 4, 8]), (4, [8, 16]), (6, [8, 16])]:
    for depth in depths:
        for trns in ([False, True] if ctype in (0, 2, 3) else [False]):
            for (w, h) in [(37, 19), (130, 70)]:
                CASES.append((ctype, depth, trns, w, h, w * h > 2000))
for h in range(1, 10):
    for w in range(1, 10):
        CASES += [(6, 8, False, w, h, False), (0, 1, False, w, h, False)]
CASES += [(2, 8, True, 1030, 66, True), (6, 8, False, 300, 520, True), (3, 4, False, 5000, 9, True)]
SUITE = ["rose", "tux"]


def case_name(c):
    return "i_t%d_d%d_%s_%dx%d" % (c[0], c[1], "trns" if c[2] else "plain", c[3], c[4])


def main():
    read = ref_reader()
    rng = np.random.default_rng(20261016)
    out = {}
    for c in CASES:
        png = make_case(c[3], c[4], c[0], c[1], c[2], rng, c[5])
        out[case_name(c) + "/png"] = np.frombuffer(png, np.uint8)
        out[case_name(c) + "/rgba"] = read(png)
    suite, inputs = np.load(os.path.join(HERE, "suite_png.npz")), np.load(os.path.join(HERE, "suite_inputs.npz"))
    for name in SUITE:
        png = reencode_suite(suite[name].tobytes(), rng)
        rgba = read(png)
        assert np.array_equal(rgba, inputs[name]), name                      # interlacing changes the file, not the pixels
        out["i_suite_%s/png" % name] = np.frombuffer(png, np.uint8)
        out["i_suite_%s/rgba" % name] = rgba
    path = os.path.join(HERE, "png_read_adam7_cases.npz")
    np.savez_compressed(path, **out)
    print(len(out) // 2, "interlaced cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

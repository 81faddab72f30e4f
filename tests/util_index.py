"""Helpers of the indexed-colour tests (tests/test_index_host.py, tests/test_index_writer_host.py, tests/test_gpu_index.py): the numpy restatement of
include/pngloss_hip.h, "Indexed-colour streams" -- np.unique on the pixel words, the palette order, the index rows, the overhead formula and the
decision --, the shapes both the CPU harness and the GPU tests run, and the builders of the two CPU harnesses.  Nothing here calls the code under
test for an expected value."""
import os
import subprocess

import numpy as np

from tests import util as U

MAX_COLORS = 256
SLOTS = 1024


def words(img):
    """the pixels of an (H, W, 4) uint8 array as little-endian uint32 words, row by row"""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    return a.reshape(-1, 4).view("<u4").reshape(-1)


def from_words(w, width, height):
    return np.ascontiguousarray(np.asarray(w, dtype="<u4").reshape(height, width)).view(np.uint8).reshape(height, width, 4)


def restate(img):
    """dict(colors, eligible, words, entries, trns_entries, plte, trns, rows, scanlines) of an (H, W, 4) uint8 image: colors is 257 for more than
    256 and 0 without pixels; the rest only for an eligible image -- the palette ascending by word, so entries that are not opaque come first"""
    w = words(img)
    pal = np.unique(w)                                                     # sorted ascending, as uint32
    colors = min(len(pal), MAX_COLORS + 1)
    out = dict(colors=colors, eligible=1 <= colors <= MAX_COLORS)
    if not out["eligible"]:
        return out
    h, wd = img.shape[:2]
    alpha = (pal >> 24).astype(np.uint8)
    trns_entries = int((alpha != 255).sum())
    assert (alpha[:trns_entries] != 255).all() and (alpha[trns_entries:] == 255).all()
    rows = np.searchsorted(pal, w).astype(np.uint8).reshape(h, wd)
    plte = np.stack([pal & 255, (pal >> 8) & 255, (pal >> 16) & 255], axis=1).astype(np.uint8).tobytes()
    out.update(words=pal, entries=len(pal), trns_entries=trns_entries, plte=plte, trns=alpha[:trns_entries].tobytes(), rows=rows,
               scanlines=b"".join(b"\0" + rows[y].tobytes() for y in range(h)))
    return out


def overhead(entries, trns_entries):
    """the PLTE and tRNS chunks: 12 bytes of framing each"""
    return 12 + 3 * entries + (12 + trns_entries if trns_entries else 0)


def keep_indexed(eligible, indexed_bytes, truecolor_bytes, entries, trns_entries):
    return bool(eligible) and indexed_bytes + overhead(entries, trns_entries) < truecolor_bytes


def table_hash(word):
    """restated from the definition in pl_index_core.h: the top 10 bits of word * 0x9E3779B1 mod 2^32"""
    return ((int(word) * 0x9E3779B1) & 0xFFFFFFFF) >> 22


def colliding_words(count, bucket, alpha=None, start=0):
    """`count` distinct words whose table hash is `bucket` (alpha: the high byte they all carry, or any)"""
    out, w = [], start
    while len(out) < count:
        cand = (w & 0xFFFFFF) | (alpha << 24) if alpha is not None else w
        if table_hash(cand) == bucket:
            out.append(cand)
        w += 1
    assert len(set(out)) == count
    return out


def shapes():
    """name -> (H, W, 4) uint8 image: the shapes the issue lists.  Deterministic."""
    rng = np.random.default_rng(23)
    opaque = lambda n: (rng.choice(1 << 24, n, replace=False).astype(np.uint32) | np.uint32(0xFF000000))
    out = {}
    out["1x1"] = from_words([0x80123456], 1, 1)
    out["1x7"] = from_words(rng.choice(opaque(3), 7), 1, 7)
    out["5x1"] = from_words(rng.choice(opaque(2), 5), 5, 1)
    five = np.concatenate([opaque(4), np.array([0x40102030], np.uint32)])
    out["130x9_five_colours"] = from_words(rng.choice(five, 130 * 9), 130, 9)          # width % 4 == 2: the dword tail
    c256 = opaque(256)
    out["16x16_256_colours"] = from_words(rng.permutation(c256), 16, 16)
    out["257x1_257_colours"] = from_words(opaque(257), 257, 1)
    out["opaque_only"] = from_words(rng.choice(opaque(17), 33 * 21), 33, 21)
    one_translucent = np.concatenate([opaque(9), np.array([0x7F010203], np.uint32)])
    w = rng.choice(one_translucent, 40 * 12)
    w[5] = 0x7F010203
    out["one_translucent"] = from_words(w, 40, 12)
    out["256_alphas_of_one_rgb"] = from_words(rng.permutation((np.arange(256, dtype=np.uint32) << 24) | np.uint32(0x00336699)).repeat(3), 48, 16)
    out["300x200_scattered_256"] = from_words(rng.choice(c256, 300 * 200), 300, 200)  # many workgroups insert the same colours at once
    out["empty"] = np.zeros((0, 0, 4), np.uint8)
    # colours that all start their probe sequence in one slot of the table, two of them translucent; and a flat image
    coll = np.array(colliding_words(38, 5, alpha=255) + colliding_words(2, 5, alpha=3), np.uint32)
    out["colliding_hash"] = from_words(rng.choice(coll, 37 * 11), 37, 11)
    out["flat_70x30"] = from_words(np.full(70 * 30, 0xFF0A0B0C, np.uint32), 70, 30)
    assert restate(out["300x200_scattered_256"])["colors"] == 256 and restate(out["257x1_257_colours"])["colors"] == 257
    assert restate(out["colliding_hash"])["colors"] == 40 and restate(out["256_alphas_of_one_rgb"])["trns_entries"] == 255
    return out


def last_pixel_images():
    """name -> 300x200 image (59 chunks of 1024 pixels): the colour that decides eligibility lies in one pixel only.  Two images have 256 opaque
    colours everywhere and a 257th in pixel (199, 299) or in pixel (0, 0); the third has 255 everywhere and its 256th only in the last pixel"""
    rng = np.random.default_rng(57)
    c = rng.choice(1 << 24, 257, replace=False).astype(np.uint32) | np.uint32(0xFF000000)
    w, h = 300, 200
    out = {}
    body = rng.choice(c[:256], w * h)
    for name, at in (("257th_in_the_last_pixel", w * h - 1), ("257th_in_the_first_pixel", 0)):
        words_ = body.copy()
        words_[at] = c[256]
        out[name] = from_words(words_, w, h)
        assert len(np.unique(words_)) == 257 and int((words_ == c[256]).sum()) == 1
    words_ = rng.choice(c[:255], w * h)
    words_[-1] = c[255]
    out["256th_in_the_last_pixel"] = from_words(words_, w, h)
    assert len(np.unique(words_)) == 256 and int((words_ == c[255]).sum()) == 1
    return out


def device_shapes():
    """name -> (H, W, 4) uint8 image: shapes for the GPU tests only, at which the loops of pl_index_rows and pl_index_count take a second trip.
    Deterministic."""
    rng = np.random.default_rng(29)
    opaque = lambda n: (rng.choice(1 << 24, n, replace=False).astype(np.uint32) | np.uint32(0xFF000000))
    five = np.concatenate([opaque(4), np.array([0x40102030], np.uint32)])
    out = {}
    out["3x1100_five_colours"] = from_words(rng.choice(five, 3 * 1100), 3, 1100)          # rows 512..1023 a second trip, 1024..1099 a ragged third
    out["4099x3_five_colours"] = from_words(rng.choice(five, 4099 * 3), 4099, 3)          # four passes of 1024 pixels and a tail of three
    out["1030x520_256_colours"] = from_words(rng.choice(opaque(256), 1030 * 520), 1030, 520)
    out.update(last_pixel_images())
    for name in ("3x1100_five_colours", "4099x3_five_colours"):
        assert restate(out[name])["colors"] == 5
    assert restate(out["1030x520_256_colours"])["colors"] == 256
    return out


ROW_BLOCKS = 512               # pl_launch_index_rows: min(height, 512) workgroups an image, each striding over the rows
ROW_PASS = 1024                # ... of 256 lanes with four pixels each, striding over a row


# ---- tests/c/index_host.cpp: the core's bodies on the CPU, under the sanitizers ----

def build_index_host(tmp_path):
    exe = str(tmp_path / "index_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "index_host.cpp"), "-lpthread"], check=True, capture_output=True)
    return exe


def run_index_host(exe, tmp_path, cases):
    """cases: (image (H, W, 4) uint8, threads).  Returns per case dict(count, entries, trns_entries, words, rows (H, pitch) uint8, pitch, ids);
    entries and what follows only where 1 <= count <= 256.  Fails on any sanitizer report."""
    path, out_path = str(tmp_path / "index_cases.bin"), str(tmp_path / "index_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for img, threads in cases:
            fh.write(np.array([img.shape[1], img.shape[0], threads], np.uint32).tobytes())
            fh.write(words(img).tobytes())
    r = subprocess.run([exe, path, out_path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    raw = np.fromfile(out_path, np.uint8)
    got, at = [], 0
    for img, _ in cases:
        h, w = img.shape[:2]
        count, entries, trns, pitch = (int(x) for x in raw[at:at + 16].view("<u4"))
        at += 16
        g = dict(count=count)
        if entries:
            g.update(entries=entries, trns_entries=trns, pitch=pitch, words=raw[at:at + 4 * entries].view("<u4").copy())
            at += 4 * entries
            g["ids"] = raw[at:at + h].copy()
            at += h
            g["rows"] = raw[at:at + h * pitch].reshape(h, pitch).copy()
            at += h * pitch
        got.append(g)
    assert at == raw.size
    return got


# ---- tests/c/index_write.c: png_stream_write with a palette ----

PNG_INC = "/opt/conda/include" if os.path.exists("/opt/conda/include/png.h") else "/usr/include"
PNG_LIB = "/lib/x86_64-linux-gnu/libpng16.so.16"
CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists(os.path.join(PNG_INC, "png.h"))


def build_index_write(tmp_path):
    exe = str(tmp_path / "index_write")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CLI, "-o", exe,
                    os.path.join(U.ROOT, "tests", "c", "index_write.c"), os.path.join(CLI, "png_stream_writer.c"), "-lz"], check=True, capture_output=True)
    return exe


def chunks_of(data):
    """[(tag, payload)] of a PNG file, CRCs checked"""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, o = [], 8
    while o < len(data):
        n, tag = struct.unpack(">I4s", data[o:o + 8])
        body = data[o + 8:o + 8 + n]
        assert struct.unpack(">I", data[o + 8 + n:o + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        o += 12 + n
    return out

"""The command line tool's container reader (pngloss_amd/cli/png_stream_reader.c: signature, chunk walk, CRCs, IHDR / PLTE / tRNS / gAMA / sRGB, zlib
inflate of the IDAT data) on hostile files, as a stand-alone program under -fsanitize=address,undefined (tests/c/png_container_main.c).  The files
are written here with struct and zlib; what the reader accepts must equal, field for field, the restatement pngloss_amd.lib.parse_png +
zlib.decompress make of the same bytes, what is damaged or unusual must be refused (the tool then reads the file with libpng), and nothing may
produce a sanitizer report.  Every case on a 3x2 and a 1x1 image of each colour type."""
import os
import struct
import subprocess
import zlib

import pytest

from pngloss_amd import lib as L
from tests import util as U
from tests import util_inflate as Z

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


def chunk(tag, body, crc_xor=0, length=None):
    return struct.pack(">I", len(body) if length is None else length) + tag + body + struct.pack(">I", (zlib.crc32(tag + body) & 0xFFFFFFFF) ^ crc_xor)


def ihdr(w, h, depth, ct, comp=0, filt=0, lace=0):
    return struct.pack(">IIBBBBB", w, h, depth, ct, comp, filt, lace)


def scanlines(w, h, depth, ct, seed=0):
    """h rows of filter type none; palette indices stay below 2 (every palette here has at least two entries... or one: index 0)"""
    rowbytes = (w * CHANNELS[ct] * depth + 7) // 8
    if ct == 3:
        return (b"\x00" + bytes(rowbytes)) * h
    return b"".join(b"\x00" + bytes((seed + 37 * r + 11 * i) & 255 for i in range(rowbytes)) for r in range(h))


def fnv(data):
    h = 0xcbf29ce484222325
    for v in data:
        h = ((h ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


PLTE2 = bytes([1, 2, 3, 250, 251, 252])


def base(ct, w, h, depth=8):
    """the chunk list of an ordinary file: [(tag, body)]"""
    out = [(b"IHDR", ihdr(w, h, depth, ct))]
    if ct == 3:
        out.append((b"PLTE", PLTE2))
    out += [(b"IDAT", zlib.compress(scanlines(w, h, depth, ct), 6)), (b"IEND", b"")]
    return out


def png(chunks):
    return SIG + b"".join(chunk(t, b) for t, b in chunks)


def insert(chunks, before, *new):
    i = [t for t, _ in chunks].index(before)
    return chunks[:i] + list(new) + chunks[i:]


def replace(chunks, tag, body):
    return [(t, body if t == tag else b) for t, b in chunks]


def cases(ct, w, h):
    """[(name, file bytes, accept, extras)]: extras = what the file holds beyond parse_png's fields (gAMA value, sRGB)"""
    out = []
    B = base(ct, w, h)
    good = png(B)
    idat = dict(B)[b"IDAT"]
    raw = scanlines(w, h, 8, ct)

    def add(name, data, accept, **extras):
        out.append(("%s_ct%d_%dx%d" % (name, ct, w, h), data, accept, extras))

    def addc(name, chunks, accept, **extras):
        add(name, png(chunks), accept, **extras)

    add("ordinary", good, True)
    # the file's size and frame
    add("file_of_0_bytes", b"", False)
    add("file_of_8_bytes", SIG, False)
    bare = SIG + chunk(b"IHDR", ihdr(w, h, 8, ct)) + chunk(b"IEND", b"")
    assert len(bare) == 45
    add("file_of_44_bytes", bare[:44], False)
    add("file_of_45_bytes", bare, False)
    add("wrong_signature", b"\x89PNG\r\n\x1a\r" + good[8:], False)
    at = good.index(b"IDAT") - 4
    add("chunk_length_beyond_the_file", good[:at] + struct.pack(">I", len(good)) + good[at + 4:], False)
    add("chunk_length_one_beyond_the_file", good[:at] + struct.pack(">I", len(idat) + 12 + 1) + good[at + 4:], False)
    add("chunk_length_0x80000000", good[:at] + struct.pack(">I", 0x80000000) + good[at + 4:], False)
    add("chunk_length_0xffffffff", good[:at] + struct.pack(">I", 0xFFFFFFFF) + good[at + 4:], False)
    # CRC off by a bit in each chunk kind (a file that has every kind its colour type allows)
    rich = insert(B, b"PLTE" if ct == 3 else b"IDAT", (b"gAMA", struct.pack(">I", 45455)), (b"sRGB", b"\x00"))
    if ct == 2:
        rich = insert(rich, b"IDAT", (b"PLTE", PLTE2))
    if ct in (0, 2, 3):
        rich = insert(rich, b"IDAT", (b"tRNS", {0: b"\x00\x07", 2: b"\x00\x01\x00\x02\x00\x03", 3: b"\x80"}[ct]))
    addc("every_chunk_kind", rich, True, gama=45455, srgb=True)
    for i, (tag, _) in enumerate(rich):
        for bit in (0, 31):
            add("crc_off_by_bit_%d_in_%s" % (bit, tag.decode()), SIG + b"".join(chunk(t, b, crc_xor=(1 << bit) if k == i else 0) for k, (t, b) in enumerate(rich)), False)
    # IHDR
    addc("ihdr_second", [(b"gAMA", struct.pack(">I", 45455))] + B, False)
    addc("ihdr_twice", B[:1] + B, False)
    addc("ihdr_of_12_bytes", replace(B, b"IHDR", ihdr(w, h, 8, ct)[:12]), False)
    addc("ihdr_of_14_bytes", replace(B, b"IHDR", ihdr(w, h, 8, ct) + b"\x00"), False)
    for name, ww, hh in (("width_0", 0, h), ("height_0", w, 0), ("width_1000001", 1000001, h), ("height_1000001", w, 1000001), ("width_0x80000000", 0x80000000, h),
                         ("rowbytes_beyond_int_max_over_height", 1000000, 537), ("a_million_each_way", 1000000, 1000000)):
        addc(name, replace(B, b"IHDR", ihdr(ww, hh, 8, ct)), False)
    addc("compression_method_1", replace(B, b"IHDR", ihdr(w, h, 8, ct, comp=1)), False)
    addc("filter_method_1", replace(B, b"IHDR", ihdr(w, h, 8, ct, filt=1)), False)
    addc("interlace_method_2", replace(B, b"IHDR", ihdr(w, h, 8, ct, lace=2)), False)
    # PLTE
    if ct == 3:
        for n, ok in ((0, False), (1, False), (767, False), (768, True), (771, False)):
            addc("plte_of_%d_bytes" % n, replace(B, b"PLTE", bytes(i & 255 for i in range(n))), ok)
        addc("plte_missing", [c for c in B if c[0] != b"PLTE"], False)
        addc("plte_twice", insert(B, b"IDAT", (b"PLTE", PLTE2)), False)
        addc("plte_behind_idat", insert([c for c in B if c[0] != b"PLTE"], b"IEND", (b"PLTE", PLTE2)), False)
    if ct == 2:
        addc("plte_present_for_rgb", insert(B, b"IDAT", (b"PLTE", PLTE2)), True)
        addc("plte_of_5_bytes_for_rgb", insert(B, b"IDAT", (b"PLTE", PLTE2[:5])), False)
        addc("plte_behind_idat_for_rgb", insert(B, b"IEND", (b"PLTE", PLTE2)), False)
    # tRNS
    if ct == 3:
        addc("trns_ok", insert(B, b"IDAT", (b"tRNS", b"\x80\x40")), True)
        addc("trns_in_front_of_plte", insert(B, b"PLTE", (b"tRNS", b"\x80")), False)
        addc("trns_longer_than_the_palette", insert(B, b"IDAT", (b"tRNS", b"\x80\x40\x20")), False)
        addc("trns_of_257_bytes", insert(replace(B, b"PLTE", bytes(768)), b"IDAT", (b"tRNS", bytes(257))), False)
    if ct == 0:
        addc("trns_ok", insert(B, b"IDAT", (b"tRNS", b"\x00\x07")), True)
        for n in (0, 1, 3):
            addc("trns_of_%d_bytes_for_gray" % n, insert(B, b"IDAT", (b"tRNS", bytes(n))), False)
    if ct == 2:
        addc("trns_ok", insert(B, b"IDAT", (b"tRNS", bytes(6))), True)
        for n in (5, 7):
            addc("trns_of_%d_bytes_for_rgb" % n, insert(B, b"IDAT", (b"tRNS", bytes(n))), False)
    if ct in (4, 6):
        addc("trns_on_a_type_with_alpha", insert(B, b"IDAT", (b"tRNS", bytes(2 if ct == 4 else 6))), False)
    t = {0: b"\x00\x07", 2: bytes(6), 3: b"\x80", 4: b"\x00\x07", 6: bytes(6)}[ct]
    addc("trns_twice", insert(B, b"IDAT", (b"tRNS", t), (b"tRNS", t)), False)
    addc("trns_behind_idat", insert(B, b"IEND", (b"tRNS", t)), False)
    # gAMA, sRGB, other chunks
    addc("gama_ok", insert(B, b"PLTE" if ct == 3 else b"IDAT", (b"gAMA", struct.pack(">I", 100000))), True, gama=100000)
    addc("gama_of_0", insert(B, b"PLTE" if ct == 3 else b"IDAT", (b"gAMA", struct.pack(">I", 0))), False)
    addc("gama_of_3_bytes", insert(B, b"PLTE" if ct == 3 else b"IDAT", (b"gAMA", b"\x00\x01\x02")), False)
    addc("gama_twice", insert(B, b"PLTE" if ct == 3 else b"IDAT", (b"gAMA", struct.pack(">I", 45455)), (b"gAMA", struct.pack(">I", 45455))), False)
    addc("gama_behind_idat", insert(B, b"IEND", (b"gAMA", struct.pack(">I", 45455))), False)
    if ct in (2, 3):
        P = B if ct == 3 else insert(B, b"IDAT", (b"PLTE", PLTE2))
        addc("gama_behind_plte", insert(P, b"IDAT", (b"gAMA", struct.pack(">I", 45455))), False)
    addc("srgb_ok", insert(B, b"IDAT", (b"sRGB", b"\x01")), True, srgb=True)
    addc("srgb_of_2_bytes", insert(B, b"IDAT", (b"sRGB", b"\x01\x00")), False)
    addc("srgb_of_0_bytes", insert(B, b"IDAT", (b"sRGB", b"")), False)
    addc("unknown_ancillary_chunk", insert(B, b"IDAT", (b"tEXt", b"Title\x00x")), False)
    addc("unknown_critical_chunk", insert(B, b"IDAT", (b"ABCD", b"")), False)
    # IDAT, IEND
    others = [c for c in B if c[0] not in (b"IDAT", b"IEND")]
    addc("idat_in_1_byte_chunks", others + [(b"IDAT", idat[i:i + 1]) for i in range(len(idat))] + [(b"IEND", b"")], True)
    addc("idat_split_by_another_chunk", others + [(b"IDAT", idat[:3]), (b"sRGB", b"\x00"), (b"IDAT", idat[3:]), (b"IEND", b"")], False)
    addc("empty_idat_in_front", insert(B, b"IDAT", (b"IDAT", b"")), True)
    addc("empty_idat_behind", insert(B, b"IEND", (b"IDAT", b"")), True)
    addc("no_idat", [c for c in B if c[0] != b"IDAT"], False)
    addc("only_an_empty_idat", replace(B, b"IDAT", b""), False)
    addc("no_iend", B[:-1], False)
    add("iend_cut_in_its_crc", good[:-1], False)
    add("bytes_behind_iend", good + b"\x00", False)
    add("a_chunk_behind_iend", good + chunk(b"IDAT", b""), False)
    # the zlib stream
    addc("stream_one_scanline_byte_short", replace(B, b"IDAT", zlib.compress(raw[:-1], 6)), False)
    addc("stream_one_scanline_byte_long", replace(B, b"IDAT", zlib.compress(raw + b"\x00", 6)), False)
    addc("stream_with_a_byte_behind_its_trailer", replace(B, b"IDAT", idat + b"\x00"), False)
    addc("stream_with_a_wrong_adler", replace(B, b"IDAT", idat[:-1] + bytes([idat[-1] ^ 1])), False)
    addc("stream_cut_in_its_trailer", replace(B, b"IDAT", idat[:-1]), False)
    addc("stream_stored", replace(B, b"IDAT", zlib.compress(raw, 0)), True)
    return out


def formats():
    """every colour type x bit depth pair: the ones PNG allows with scanlines of their size (accepted), the others with the 8-bit file's (refused)"""
    out = []
    for w, h in ((3, 2), (1, 1)):
        for ct in range(8):
            for depth in (0, 1, 2, 3, 4, 8, 16, 32):
                ok = depth in DEPTHS.get(ct, ())
                chunks = base(ct, w, h, depth) if ok else replace(base(ct if ct in CHANNELS else 0, w, h), b"IHDR", ihdr(w, h, depth, ct))
                if not ok and ct == 3:
                    chunks = insert([c for c in chunks if c[0] != b"PLTE"], b"IDAT", (b"PLTE", PLTE2))
                out.append(("format_ct%d_depth%d_%dx%d" % (ct, depth, w, h), png(chunks), ok, {}))
    return out


def restate(data, extras):
    """what the reader's line must say for an accepted file: parse_png + zlib.decompress of the same bytes"""
    p = L.parse_png(data)
    sl = zlib.decompress(p["zstream"])
    plte, trns = p["plte"] or b"", p["trns"]
    return "accept %d %d %d %d %d %d %s %d %s %d %d %d %d %d %016x %d" % (
        p["width"], p["height"], p["ctype"], p["depth"], p["interlace"], len(plte) // 3, plte.hex() or "-", len(trns or b""), (trns or b"").hex() or "-",
        trns is not None, bool(extras.get("srgb")), "gama" in extras, extras.get("gama", 0), len(sl), fnv(sl), len(data))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("png_container") / "png_container_main")
    r = subprocess.run(["gcc", "-std=gnu11"] + Z.SANITIZE + ["-o", exe, os.path.join(U.ROOT, "tests", "c", "png_container_main.c"),
                        os.path.join(U.ROOT, "pngloss_amd", "cli", "png_stream_reader.c"), "-lz", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _check(program, tmp_path, all_cases):
    paths = []
    for i, (name, data, _, _) in enumerate(all_cases):
        paths.append(str(tmp_path / ("%04d.png" % i)))
        with open(paths[-1], "wb") as fh:
            fh.write(data)
    lines = Z.run_sanitized([program] + paths).splitlines()
    assert len(lines) == len(all_cases)
    for (name, data, accept, extras), line in zip(all_cases, lines):
        assert line == (restate(data, extras) if accept else "refuse"), name
    return lines


@pytest.mark.parametrize("shape", [(3, 2), (1, 1)])
def test_container_reader_on_hostile_files(program, tmp_path, shape):
    """Every case of the list on an image of each colour type: accepted files equal the restatement field for field, the others are refused, the
    sanitizers stay silent."""
    all_cases = [c for ct in (0, 2, 3, 4, 6) for c in cases(ct, *shape)]
    assert len({c[0] for c in all_cases}) == len(all_cases)
    lines = _check(program, tmp_path, all_cases)
    print("%dx%d: %d files, %d accepted" % (shape + (len(lines), sum(ln != "refuse" for ln in lines))))
    assert sum(c[2] for c in all_cases) >= 40


def test_container_reader_colour_type_and_depth_pairs(program, tmp_path):
    """Every colour type 0..7 x bit depth pair: the fifteen PNG allows are accepted with scanlines of their size, every other pair is refused."""
    all_cases = formats()
    lines = _check(program, tmp_path, all_cases)
    assert sum(ln != "refuse" for ln in lines) == 2 * 15

"""CPU tests of the option "index_depth" (no GPU): the body of pl_index_pack, the rule that names the stream to keep and the layout of the packed
rows (pngloss_amd/csrc/pl_index_core.h, pl_layout.h) run under the sanitizers by tests/c/index_depth_host.cpp, against the numpy restatement of
tests/util_index_depth.py; the binding tables against include/pngloss_hip_index_depth.h; and the condition on the inputs the GPU tests rely on."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util as U
from tests import util_index as X
from tests import util_index_depth as D

WIDTHS = list(range(1, 71)) + [255, 256, 257]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build_index_depth_host(tmp_path_factory.mktemp("index_depth_host"))


def test_restatement_arithmetic():
    assert [D.min_depth(e) for e in (0, 1, 2, 3, 4, 5, 16, 17, 256, 257)] == [0, 1, 1, 2, 2, 4, 4, 8, 8, 0]
    # PNG's own example layout: the leftmost pixel in the high bits
    assert D.pack_rows(np.array([[1, 0, 0, 0, 0, 0, 0, 1, 1]], np.uint8), 1).tolist() == [[0x81, 0x80]]
    assert D.pack_rows(np.array([[3, 0, 1, 2, 2]], np.uint8), 2).tolist() == [[0xC6, 0x80]]
    assert D.pack_rows(np.array([[15, 1, 7]], np.uint8), 4).tolist() == [[0xF1, 0x70]]
    assert D.scanlines(np.array([[1, 1], [0, 1]], np.uint8), 1) == b"\x00\xc0\x00\x40"
    rng = np.random.default_rng(3)
    for depth in (1, 2, 4):
        rows = rng.integers(0, 1 << depth, (3, 37)).astype(np.uint8)
        assert np.array_equal(D.unpack_rows(D.pack_rows(rows, depth), 37, depth), rows)
    assert D.trip_pixels(1) == 8192 and D.trip_pixels(2) == 4096 and D.trip_pixels(4) == 2048


def test_pack_body_equals_both_restatements(exe, tmp_path):
    """every depth at every width 1..70 and 255, 256, 257, three rows each: random indices, and every index at its largest value.  The harness
    fills the 8-bit rows behind `width` with 0xFF, ends their allocation with the last row's pitch, and holds the result against its own
    one-pixel-at-a-time restatement; here the same bytes are held against numpy's."""
    rng = np.random.default_rng(41)
    cases = []
    for depth in (1, 2, 4):
        top = (1 << depth) - 1
        for w in WIDTHS:
            cases.append((depth, rng.integers(0, top + 1, (3, w)).astype(np.uint8)))
            cases.append((depth, np.full((3, w), top, np.uint8)))
    for (depth, rows), (pitch8, pitch, got) in zip(cases, D.run_pack(exe, tmp_path, cases)):
        w = rows.shape[1]
        want = D.pack_rows(rows, depth)
        nbytes, dwords = (w * depth + 7) // 8, (w * depth + 31) // 32
        assert want.shape[1] == nbytes
        assert pitch8 % 16 == 0 and pitch8 >= w and pitch % 16 == 0 and pitch >= 4 * dwords, (depth, w)
        assert np.array_equal(got[:, :nbytes], want), (depth, w)
        assert not got[:, nbytes:4 * dwords].any(), (depth, w)             # the tail of the last dword
        assert (got[:, 4 * dwords:] == 0xEE).all(), (depth, w)             # nothing is written beyond it
        if w % (8 // depth):                                               # the unused low bits of the last byte
            assert not (got[:, nbytes - 1] & ((1 << (8 - (w * depth) % 8)) - 1)).any(), (depth, w)


def test_min_depth(exe):
    got = [int(x) for x in D.run_harness(exe, ["min_depth"]).split()]
    assert got == [D.min_depth(e) for e in range(258)]
    assert got[0] == 0 and got[257] == 0 and got[1:3] == [1, 1] and got[3:5] == [2, 2] and set(got[5:17]) == {4} and set(got[17:257]) == {8}


def test_rule_in_every_ordering_and_tie(exe):
    """(T, I8 + overhead, Ip + overhead) in every order and with every tie, for min_depth 1, 2, 4 and 8, images that are not eligible, with and
    without tRNS, in the three modes"""
    lines, want = [], []
    for mode, colors, trns in itertools.product(("8", "auto", "min"), (0, 1, 2, 3, 4, 5, 16, 17, 256, 257), (0, 1)):
        ov = X.overhead(colors, trns)
        for costs in itertools.product((1000, 1001, 1002), repeat=3):     # every ordering of three costs, every tie among them
            T, I8, Ip = costs[0] + ov, costs[1], costs[2]
            lines.append(f"{D.MODES[mode]} {colors} {T} {I8} {Ip} {trns}")
            md = D.min_depth(colors)
            has8, hasp = bool(md) and (mode != "min" or md == 8), bool(md) and mode != "8" and md < 8
            want.append(D.choose(mode, colors, T, I8, Ip, trns) + (int(has8), int(hasp)))
    got = [tuple(int(x) for x in line.split()) for line in D.run_harness(exe, ["rule"], "\n".join(lines) + "\n").splitlines()]
    assert len(got) == len(want) == 3 * 10 * 2 * 27
    assert got == want
    # spelled out: "auto" keeps the earlier candidate on a tie, "min" never looks at I8 below 17 colours, "8" never at Ip
    ov = X.overhead(4, 0)
    assert D.choose("auto", 4, 100 + ov, 100, 100, 0) == (0, 100) and D.choose("auto", 4, 101 + ov, 100, 100, 0) == (8, 100)
    assert D.choose("auto", 4, 101 + ov, 100, 99, 0) == (2, 99) and D.choose("auto", 4, 100 + ov, 100, 99, 0) == (2, 99)
    assert D.choose("min", 4, 101 + ov, 1, 100, 0) == (2, 100) and D.choose("min", 4, 100 + ov, 1, 100, 0) == (0, 100)
    assert D.choose("8", 4, 101 + ov, 100, 1, 0) == (8, 100) and D.choose("min", 17, 101 + X.overhead(17, 0), 100, 1, 0) == (8, 100)
    assert D.choose("auto", 257, 5, 1, 1, 0) == (0, 0) and D.choose("auto", 0, 0, 0, 0, 0) == (0, 0)


@pytest.mark.parametrize("dims", [[], [(0, 0)], [(5, 0), (0, 7)], [(1, 1)], [(7, 3), (0, 0), (33, 2), (8193, 2), (5, 600), (256, 256), (31, 1)]])
def test_layout_of_the_packed_rows(exe, dims):
    flat = [v for wh in dims for v in wh]
    lines = [[int(x) for x in line.split()] for line in D.run_harness(exe, ["layout"] + flat).splitlines()]
    (index_total, jobs, total), images = lines[0], lines[1:]
    assert len(images) == len(dims)
    assert jobs % 256 == 0 and jobs >= index_total and total % 256 == 0       # behind everything pl_index_layout laid out
    regions = [(jobs, D.PACK_JOB_BYTES * max(len(dims), 1))]
    for (w, h), (ids, rows, pitch, rows8, pitch8) in zip(dims, images):
        assert ids % 256 == 0 and rows % 256 == 0
        if w and h:
            for depth in (1, 2, 4):
                assert pitch >= ((w * depth + 7) // 8 + 3) // 4 * 4
            assert pitch % 16 == 0 and pitch8 % 16 == 0
            regions += [(ids, h), (rows, pitch * h)]
            assert rows8 + pitch8 * h <= index_total
        else:
            assert pitch == 0
    regions.sort()
    for (a, an), (b, _) in zip(regions, regions[1:]):
        assert a + an <= b
    assert all(at >= index_total for at, _ in regions) and regions[-1][0] + regions[-1][1] <= total


def test_binding_tables_of_the_extension_header(tmp_path):
    """pngloss_amd.lib.INDEX_DEPTH_STRUCTS and INDEX_DEPTH_PROTOTYPES against what the compiler makes of include/pngloss_hip_index_depth.h"""
    from pngloss_amd import lib as L
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_index_depth.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.INDEX_DEPTH_PROTOTYPES) == ["pngloss_hip_last_index_depth", "pngloss_hip_multi_last_index_depth"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.INDEX_DEPTH_STRUCTS) == ["pngloss_hip_index_depth"]
    assert '#include "pngloss_hip_indexed.h"' in header
    taken = (set(L.PROTOTYPES) | set(L.INDEXED_PROTOTYPES) | set(L.QUANT_PROTOTYPES) | set(L.DITHER_PROTOTYPES) | set(L.QUANT_TARGET_PROTOTYPES)
             | set(L.QUANT_SPACE_PROTOTYPES))
    assert not set(L.INDEX_DEPTH_PROTOTYPES) & taken

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    name, cls = "pngloss_hip_index_depth", L.IndexDepth
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_index_depth.h"', "int main(void) {",
             f'    printf("{name} . %zu 0\\n", sizeof({name}));']
    lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    seen = 0
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        _, field, size, offset = line.split()
        mine = (L.C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        assert mine == (int(size), int(offset)), field
        seen += 1
    assert seen == 1 + len(cls._fields_)
    assert [f for f, _ in cls._fields_] == ["bit_depth", "min_depth", "indexed8_bytes", "packed_bytes"] and L.C.sizeof(cls) == 24
    # the older records keep their size: this one stands beside them
    assert L.C.sizeof(L.Palette) == 8 + 768 + 256 + 16 + 8

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_index_depth.h"
template <class T> void put() {
    if constexpr (std::is_void_v<T>) std::printf(" void");
    else if constexpr (std::is_pointer_v<T>) std::printf(" ptr");
    else if constexpr (std::is_integral_v<T>) std::printf(" %c%zu", std::is_signed_v<T> ? 'i' : 'u', sizeof(T) * 8);
    else std::printf(" other");
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void show(const char *name) { std::printf("%s", name); put<R>(); (put<A>(), ...); std::printf("\\n"); }
};
int main() {
""" + "".join(f'    Sig<decltype(&{fn})>::show("{fn}");\n' for fn in functions) + "    return 0;\n}\n"
    declared = {line.split()[0]: line.split()[1:] for line in run("prototypes.cpp", text, ["g++", "-std=c++17"]).splitlines()}
    assert declared["pngloss_hip_last_index_depth"] == ["i32", "ptr", "u64", "ptr"]
    assert prototype_differences(L.INDEX_DEPTH_PROTOTYPES, declared) == []
    import pngloss_amd as P
    for fn in functions:                                             # the library exports both, and hip_lib() has given them their prototypes
        assert getattr(P.hip_lib(), fn).argtypes == L.INDEX_DEPTH_PROTOTYPES[fn][1]


def test_noise_inputs_pack_smaller_with_zlib_9():
    """what the GPU tests rely on, recorded with zlib level 9 on the CPU: on the noise inputs the packed rows plus overhead are at most 0.9 times
    the 8-bit rows plus overhead, and 0.9 times the best of filter 0 / 1 / 2 truecolour rows"""
    for name, img in D.noise_inputs().items():
        T, I8, Ip, ov, md = D.zlib9_sizes(img)
        print(name, "min_depth", md, "T", T, "I8", I8, "Ip", Ip, "overhead", ov, "ratio to I8", round((Ip + ov) / (I8 + ov), 3), "to T", round((Ip + ov) / T, 3))
        assert md == D.min_depth(int(name.split("_")[1])) and md < 8
        assert Ip + ov <= 0.9 * (I8 + ov), name
        assert Ip + ov <= 0.9 * T, name
    for name, img in D.structured_inputs().items():
        T, I8, Ip, ov, md = D.zlib9_sizes(img)
        print(name, "min_depth", md, "T", T, "I8", I8, "Ip", Ip, "overhead", ov)


# ---- the container: png_stream_write below 8 bits, read back through the tool's own libpng bridge ----

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
needs_png = pytest.mark.skipif(not (X.have_png and os.path.exists(X.PNG_LIB)), reason="libpng headers/runtime not found on this box")


@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("index_depth_write") / "index_depth_write")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + X.PNG_INC, "-I" + CLI,
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", "index_depth_write.c"), os.path.join(CLI, "png_stream_writer.c"), os.path.join(CLI, "png_bridge.c"),
                    X.PNG_LIB, "-lz", "-lm"], check=True, capture_output=True)
    return exe


def _palette_image(entries, trns_entries, width, height, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.choice(1 << 24, entries, replace=False).astype(np.uint32)
    alpha = np.concatenate([rng.integers(0, 255, trns_entries), np.full(entries - trns_entries, 255)]).astype(np.uint32)
    pal = np.sort(rgb | (alpha << 24))
    idx = rng.integers(0, entries, (height, width)).astype(np.uint8)
    idx[-1, -1] = entries - 1                                               # the largest index, in the row's last pixel
    plte = np.stack([pal & 255, (pal >> 8) & 255, (pal >> 16) & 255], axis=1).astype(np.uint8).tobytes()
    return pal, idx, plte, ((pal >> 24).astype(np.uint8)[:trns_entries]).tobytes()


def _write(writer, tmp_path, width, height, bits, plte, trns, rows, stream=None):
    for name, data in (("plte.bin", plte), ("trns.bin", trns), ("rows.bin", rows), ("z.bin", stream or b"")):
        (tmp_path / name).write_bytes(data)
    out, raw = tmp_path / "out.png", tmp_path / "out.rgba"
    for p in (out, raw):
        if p.exists():
            p.unlink()
    r = subprocess.run([writer, str(out), str(raw), str(width), str(height), str(bits), str(tmp_path / "plte.bin"), str(tmp_path / "trns.bin") if trns else "-",
                        str(tmp_path / "rows.bin"), str(tmp_path / "z.bin") if stream else "-"], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    rc, written, predicted, read_rc = (int(v) for v in r.stdout.split())
    return rc, written, predicted, read_rc, (out.read_bytes() if out.exists() else b""), (np.fromfile(raw, np.uint8) if raw.exists() else None)


@needs_png
def test_packed_palette_files_read_back_as_the_pixels_the_palette_implies(writer, tmp_path):
    import zlib
    for depth in (1, 2, 4):
        for width in range(1, 10):
            for trns_entries in (0, 1):
                entries, height = 1 << depth, 3
                pal, idx, plte, trns = _palette_image(entries, trns_entries, width, height, seed=100 * depth + 10 * width + trns_entries)
                packed = D.pack_rows(idx, depth)
                what = (depth, width, trns_entries)
                # once deflated by the writer from the rows, once framed around a finished stream
                for stream in (None, zlib.compress(D.scanlines(idx, depth), 9)):
                    rc, written, predicted, read_rc, data, rgba = _write(writer, tmp_path, width, height, depth, plte, trns, packed.tobytes(), stream)
                    assert rc == 0 and read_rc == 0 and written == len(data), what
                    ch = dict(X.chunks_of(data))
                    assert ch[b"IHDR"][8:10] == bytes([depth, 3]) and ch[b"PLTE"] == plte and ch.get(b"tRNS", b"") == trns, what
                    assert zlib.decompress(ch[b"IDAT"]) == D.scanlines(idx, depth), what
                    if stream:
                        assert ch[b"IDAT"] == stream and predicted == len(data), what     # png_stream_file_size does not depend on the depth
                    assert np.array_equal(rgba.view("<u4").reshape(height, width), pal[idx]), what


@needs_png
def test_index_bits_0_and_8_write_the_file_as_before(writer, tmp_path):
    """a field left at 0 by a designated initialiser: the 8-bit file, byte for byte what the chunks of such a file are"""
    import struct
    import zlib
    pal, idx, plte, trns = _palette_image(16, 1, 7, 3, seed=5)
    stream = zlib.compress(D.scanlines(idx, 8), 9)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    want = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 3, 8, 3, 0, 0, 0)) + chunk(b"PLTE", plte) + chunk(b"tRNS", trns) + chunk(b"IDAT", stream)
            + chunk(b"IEND", b""))
    for bits in (0, 8):
        rc, written, predicted, read_rc, data, rgba = _write(writer, tmp_path, 7, 3, bits, plte, trns, idx.tobytes(), stream)
        assert rc == 0 and read_rc == 0 and data == want and written == predicted == len(want), bits
        assert np.array_equal(rgba.view("<u4").reshape(3, 7), pal[idx])
    # without a finished stream the writer deflates width bytes a row, as before
    zero, eight = (_write(writer, tmp_path, 7, 3, bits, plte, trns, idx.tobytes())[4] for bits in (0, 8))
    assert zero == eight and zlib.decompress(dict(X.chunks_of(zero))[b"IDAT"]) == D.scanlines(idx, 8)


@needs_png
def test_depths_and_palettes_that_cannot_be_written_are_refused(writer, tmp_path):
    pal, idx, plte, trns = _palette_image(2, 0, 5, 2, seed=6)
    rows = D.pack_rows(idx, 1).tobytes()
    for bits in (3, 16, 5, 7, 32):
        assert _write(writer, tmp_path, 5, 2, bits, plte, trns, rows)[0] == 4, bits           # INVALID_ARGUMENT
    pal3, idx3, plte3, _ = _palette_image(3, 0, 5, 2, seed=7)
    assert _write(writer, tmp_path, 5, 2, 1, plte3, b"", D.pack_rows(idx3 & 1, 1).tobytes())[0] == 4      # 3 entries at 1 bit
    assert _write(writer, tmp_path, 5, 2, 2, plte3, b"", D.pack_rows(idx3, 2).tobytes())[0] == 0
    pal17, idx17, plte17, _ = _palette_image(17, 0, 5, 2, seed=8)
    assert _write(writer, tmp_path, 5, 2, 4, plte17, b"", D.pack_rows(idx17 & 15, 4).tobytes())[0] == 4
    pal5, idx5, plte5, _ = _palette_image(5, 0, 5, 2, seed=9)
    assert _write(writer, tmp_path, 5, 2, 2, plte5, b"", D.pack_rows(idx5 & 3, 2).tobytes())[0] == 4


# ---- the switch --index-depth and its -v line, without I/O ----

@pytest.fixture(scope="module")
def cli_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cli_index_depth") / "cli_index_depth_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_index_depth_host.c"),
                    os.path.join(CLI, "cli_options.c"), os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)
    return exe


def _cli(exe, args, cwd):
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


def test_switch_needs_a_palette_switch_and_one_of_three_values(cli_host, tmp_path):
    for value in ("auto", "min", "8"):
        r = _cli(cli_host, ["--index-depth", value, "x.png"], tmp_path)
        assert r.returncode == 4 and r.stderr == "--index-depth requires --indexed or --colors.\n", (value, r.stderr)
        for palette in (["--indexed"], ["--colors", "16"], ["--colors", "2", "--dither"]):
            r = _cli(cli_host, palette + ["--index-depth", value, "x.png"], tmp_path)
            f = _fields(r.stdout)
            assert r.returncode == 0 and f["have_index_depth"] == "1" and f["index_depth"] == value and f["indexed"] == "1" and f["gpu_deflate"] == "1", r.stderr
    for value in ("4", "1", "2", "16", "AUTO", "", "max", "8 "):
        r = _cli(cli_host, ["--colors", "16", "--index-depth", value, "x.png"], tmp_path)
        assert r.returncode == 4 and r.stderr == "--index-depth requires auto, min or 8\n", (value, r.stderr)
    r = _cli(cli_host, ["--indexed", "--index-depth"], tmp_path)          # getopt's own message
    assert r.returncode == 4
    assert not os.listdir(tmp_path)
    # without the switch nothing is set, and the older rules answer first
    f = _fields(_cli(cli_host, ["--colors", "16", "x.png"], tmp_path).stdout)
    assert f["have_index_depth"] == "0" and f["index_depth"] == ""
    r = _cli(cli_host, ["--dither", "--index-depth", "auto", "x.png"], tmp_path)
    assert r.returncode == 4 and r.stderr == "--dither requires --colors.\n"
    r = _cli(cli_host, ["--indexed", "--index-depth", "bad", "--target-size", "10k", "x.png"], tmp_path)
    assert r.returncode == 4 and r.stderr.startswith("--indexed cannot be combined with")


def test_switch_is_absent_from_the_usage_text_and_named_by_the_documents(cli_host):
    import json
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        rec = {tuple(v["args"]): v for v in json.load(fh)["vectors"]}
    usage = subprocess.run([cli_host, "usage"], capture_output=True, text=True, check=True).stdout
    assert "--index-depth" not in usage and usage and usage in rec[("--help",)]["stdout"]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "--index-depth" in open(os.path.join(U.ROOT, doc)).read(), doc
    assert "pngloss_hip_index_depth.h" in open(os.path.join(U.ROOT, "INTEGRATION.md")).read()
    assert "pl_index_pack" in open(os.path.join(U.ROOT, "DESIGN.md")).read()


def test_report_line(cli_host):
    for rec in (dict(bit_depth=4, min_depth=4, indexed8_bytes=37991, packed_bytes=33045), dict(bit_depth=1, min_depth=1, indexed8_bytes=0, packed_bytes=587),
                dict(bit_depth=8, min_depth=4, indexed8_bytes=10, packed_bytes=20), dict(bit_depth=0, min_depth=2, indexed8_bytes=10, packed_bytes=20),
                dict(bit_depth=2, min_depth=2, indexed8_bytes=2 ** 40, packed_bytes=2 ** 40 - 1)):
        got = subprocess.run([cli_host, "report"] + [str(rec[k]) for k in ("bit_depth", "min_depth", "indexed8_bytes", "packed_bytes")], capture_output=True, text=True, check=True).stdout
        assert got == D.report_line(rec), rec
    assert D.report_line(dict(bit_depth=4, min_depth=4, indexed8_bytes=37991, packed_bytes=33045)) == \
        "  index depth: 4 bits, 33045 bytes of packed image data against 37991 bytes at 8 bits\n"

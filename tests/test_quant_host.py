"""CPU tests of the colour quantiser (no GPU): the kernels' logic and the host's median cut (pngloss_amd/csrc/pl_quant_core.h) run on the CPU under
the sanitizers -- with one thread, and with a team of host threads that accumulate concurrently -- against the restatement of tests/util_quant.py;
the median cut's tie rules on hand-made histograms; the 2^24-pixel bound of a workgroup and the 2^32 - 1 pixels of an image as arithmetic; the workspace layout; the binding tables
against the compiler's view of include/pngloss_hip_quant.h; the argument checks that need no device; the switch --colors; and the restatement's
quality against Pillow's quantiser."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_quant as Q

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
INVALID = L.PNGLOSS_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return Q.build_quant_host(tmp_path_factory.mktemp("quant_host"))


@pytest.fixture(scope="module")
def want():
    """the restatement of every shape, computed once"""
    return {name: Q.restate(img, n, rounds) for name, (img, n, rounds) in Q.shapes().items()}


def _check_case(name, case, got, want):
    img, n, rounds = case
    assert np.array_equal(got["pixels"], want["pixels"]), name
    w = Q.words(img)
    assert got["hist_nonzero"] == int((Q.histogram(w) > 0).sum()) and got["hist_sum"] == w.size, name
    if want["exact"]:
        assert got["first"] == [] and np.array_equal(got["pixels"], img), name
        return
    first = Q.median_cut(Q.histogram(w), n)
    assert got["first"] == first and 1 <= len(first) <= n, name
    colours, counts = np.unique(w, return_counts=True)
    assert got["final"] == Q.refine(colours, counts.astype(np.int64), first, rounds), name
    assert sorted(set(int(x) for x in Q.words(got["pixels"]))) == want["palette"], name


def test_core_equals_the_restatement_with_one_thread(exe, tmp_path, want):
    shapes = Q.shapes()
    got = Q.run_quant_host(exe, tmp_path, [(img, n, r, 1) for img, n, r in shapes.values()])
    for (name, case), g in zip(shapes.items(), got):
        _check_case(name, case, g, want[name])


def test_core_equals_the_restatement_with_a_team_that_accumulates_concurrently(exe, tmp_path, want):
    """3, 8 and 13 host threads: groups of four share one set of 32-bit cells and every group flushes into the same 64-bit accumulators"""
    shapes = Q.shapes()
    cases = [(img, n, r, t) for t in (3, 8, 13) for img, n, r in shapes.values()]
    for k, g in enumerate(Q.run_quant_host(exe, tmp_path, cases)):
        name = list(shapes)[k % len(shapes)]
        _check_case(name, shapes[name], g, want[name])


def test_the_tie_of_the_three_colour_case_is_real(want):
    """after the first round the entries' red is 24 and 72 and the pixel 48 lies in the middle: it goes to entry 0, whose word it gets"""
    img, n, rounds = Q.shapes()["three_colours_one_equidistant"]
    assert want["three_colours_one_equidistant"]["palette"] == [0xFF000018, 0xFF000048]
    out = Q.words(want["three_colours_one_equidistant"]["pixels"])
    assert list(out) == [0xFF000018, 0xFF000048, 0xFF000018, 0xFF000018, 0xFF000048, 0xFF000048, 0xFF000018]
    assert (48 - 24) ** 2 == (72 - 48) ** 2
    assert want["three_colours_no_rounds"]["palette"] == [0xF8080820, 0xF8080848]      # R = 0: the median cut's own colours


def _word(r, g, b, a):
    return r | g << 8 | b << 16 | a << 24


def _bin(r, g, b, a):
    return r | g << 4 | b << 8 | a << 12


def test_median_cut_tie_rules_on_hand_made_histograms(exe, tmp_path):
    def both(hist, n):
        full = np.zeros(Q.BINS, np.int64)
        for b, c in hist.items():
            full[b] = c
        trace = []
        mine = Q.median_cut(full, n, trace)
        assert Q.cut_host(exe, tmp_path, hist, n) == mine
        return mine, trace

    # equal counts: two boxes of 10 pixels after the first split, both with a range -- the FIRST in the list is split next
    hist = {_bin(0, 0, 0, 15): 5, _bin(2, 0, 0, 15): 5, _bin(8, 0, 0, 15): 5, _bin(10, 0, 0, 15): 5}
    pal, trace = both(hist, 3)
    assert trace == [(0, 0, 2), (0, 0, 0)] and len(pal) == 3
    assert pal == [_word(8, 8, 8, 248), _word(40, 8, 8, 248), _word((2 * (5 * 136 + 5 * 168) + 10) // 20, 8, 8, 248)]
    # equal ranges: red and blue both span 4 -- the LOWEST channel is cut
    hist = {_bin(1, 0, 3, 15): 4, _bin(5, 0, 7, 15): 4}
    pal, trace = both(hist, 2)
    assert trace == [(0, 0, 1)] and pal == [_word(24, 8, 56, 248), _word(88, 8, 120, 248)]
    # ... and the largest range wins over a lower channel
    pal, trace = both({_bin(1, 0, 3, 15): 4, _bin(2, 0, 7, 15): 4}, 2)
    assert trace == [(0, 2, 3)]
    # no value of lo .. hi-1 reaches half: the cut is hi-1
    pal, trace = both({_bin(0, 0, 0, 0): 1, _bin(3, 0, 0, 0): 1, _bin(9, 0, 0, 0): 10}, 2)
    assert trace == [(0, 0, 8)] and pal == [_word((2 * (8 + 56) + 2) // 4, 8, 8, 8), _word(152, 8, 8, 8)]
    # a box of one bin has no range and is never split, however many pixels it has; fewer bins than N: the cut stops early
    pal, trace = both({_bin(4, 4, 4, 4): 1000, _bin(0, 0, 0, 0): 1, _bin(1, 0, 0, 0): 1}, 8)
    assert len(pal) == 3 and trace == [(0, 0, 3), (0, 0, 0)]      # (all four ranges are 4: red is cut, at hi-1; then the two-pixel box, the only one with a range)
    pal, trace = both({_bin(7, 7, 7, 7): 12}, 256)
    assert pal == [_word(120, 120, 120, 120)] and trace == []


def test_a_workgroup_never_takes_more_than_2_to_the_24_pixels(exe):
    """arithmetic, not a run: the grid the launch picks (plq_blocks) against the restated rule, and the pixels of its busiest workgroup against
    the bound that keeps 255 * pixels inside a 32-bit cell"""
    assert 255 * Q.WG_PIXELS < 1 << 32 <= 256 * Q.WG_PIXELS + (1 << 24)
    sizes = [1, 3, 1023, 1024, 1025, 8481, 1 << 20, 4096 * 4096, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 3 << 24, (1 << 30) + 5, Q.MAX_PIXELS, 1 << 32, (511 << 24) + 1,
             (512 << 24) + 1, (1 << 34) - 1, 1 << 34]
    args = [str(v) for p in sizes for want in (1, 8, 2048) for v in (p, want)]
    lines = subprocess.run([exe, "grid"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1].split() == ["limits", str(Q.WG_PIXELS), str(Q.MAX_BLOCKS), str(Q.MAX_PIXELS)]
    assert Q.MAX_PIXELS <= Q.WG_PIXELS * Q.MAX_BLOCKS               # (the grid rule holds for every size below: past the largest image that is taken)
    assert len(lines) == 3 * len(sizes) + 1
    for line in lines[:-1]:
        pixels, want, blocks, busiest = (int(x) for x in line.split())
        assert blocks == Q.blocks(pixels, want) and busiest == Q.wg_pixels(pixels, blocks), line
        assert 1 <= blocks <= Q.MAX_BLOCKS and busiest <= Q.WG_PIXELS and blocks * busiest >= pixels, line


def test_an_images_pixel_count_fits_a_histogram_bin(exe):
    """the size predicate of the argument checks (plq_pixels_ok) at its boundary: a bin of the histogram is a 32-bit count and one bin may take every
    pixel, so 2^32 - 1 pixels are the most.  Arithmetic on the CPU only: a device test of the refusal would hand an unfixed library 16 GiB to read"""
    assert Q.MAX_PIXELS == 0xFFFFFFFF and 65535 * 65537 == Q.MAX_PIXELS and 3 * 5 * 17 * 257 * 65537 == Q.MAX_PIXELS
    sizes = [(0, 0), (1, 1), (70, 46), (65535, 65537), (65537, 65535), (1, 0xFFFFFFFF), (0xFFFFFFFF, 1), (255, 16843009), (65536, 65535), (65536, 65536),
             (2, 1 << 31), (1 << 31, 2), (65537, 65536), (1 << 17, 1 << 17), (0xFFFFFFFF, 0xFFFFFFFF)]
    lines = subprocess.run([exe, "pixels"] + [str(v) for s in sizes for v in s], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1].split() == ["limit", str(Q.MAX_PIXELS)] and len(lines) == len(sizes) + 1
    for (w, h), line in zip(sizes, lines):
        assert [int(x) for x in line.split()] == [w, h, w * h, int(w * h <= Q.MAX_PIXELS)], line
    verdict = {s: int(line.split()[3]) for s, line in zip(sizes, lines)}
    assert verdict[(65535, 65537)] == 1 and verdict[(1, 0xFFFFFFFF)] == 1                       # 2^32 - 1 pixels are taken
    assert verdict[(65536, 65536)] == 0 and verdict[(2, 1 << 31)] == 0                          # 2^32 are refused
    assert verdict[(0xFFFFFFFF, 0xFFFFFFFF)] == 0 and verdict[(1 << 17, 1 << 17)] == 0          # (the old bound's 2^34 too)
    # both entry points and the launches ask the predicate, and the constant is stated once
    host = open(os.path.join(CSRC, "pl_host_quant.hip")).read()
    assert "if (!plq_pixels_ok(px)) return PNGLOSS_INVALID_ARGUMENT;" in host and host.count("check_quant_sizes(images, n, pixels_of.data())") == 2
    for name in ("pl_host_quant.hip", "pl_quant.hip", "pl_quant.h"):
        assert "PLQ_MAX_PIXELS" not in open(os.path.join(CSRC, name)).read(), name
    core = open(os.path.join(CSRC, "pl_quant_core.h")).read()
    assert len(re.findall(r"constexpr uint64_t PLQ_MAX_PIXELS\b", core)) == 1 and "static_assert(PLQ_MAX_PIXELS <= UINT32_MAX" in core


@pytest.mark.parametrize("inputs", [0, 1])
def test_workspace_layout_has_no_overlap_and_is_aligned(exe, inputs):
    shapes = [(70, 46), (0, 0), (1, 1), (257, 33), (5, 0)]
    out = subprocess.run([exe, "layout", str(inputs)] + [str(v) for s in shapes for v in s], capture_output=True, text=True, check=True).stdout
    regions = {name: (int(at), int(size)) for name, at, size in (line.split() for line in out.splitlines())}
    total = regions.pop("total0")[1]
    zeroed, tables, hists, pals = (regions.pop(k) for k in ("zeroed0", "tables0", "hists0", "pals0"))
    n = len(shapes)
    per_image = {k: v for k, v in regions.items() if re.match(r"(table|hist|pal|acc|out|in)\d+$", k)}
    head = {k: v for k, v in regions.items() if k not in per_image}
    assert len(per_image) == 6 * n and sorted(head) == ["counts0", "distort_jobs0", "distort_records0", "index_jobs0", "quant_jobs0", "records0"]
    for name, (at, size) in regions.items():
        assert at % 256 == 0 or name.startswith(("table", "hist", "pal", "acc")), name
        assert at % 16 == 0 and at + size <= total, name
    # what one memset zeroes: the counters, both kinds of record and every accumulator, and nothing else
    inside = lambda r, outer: outer[0] <= r[0] and r[0] + r[1] <= outer[0] + outer[1]
    for name, r in regions.items():
        if name in ("counts0", "records0", "distort_records0") or name.startswith("acc"):
            assert inside(r, zeroed), name
        elif r[1]:
            assert r[0] + r[1] <= zeroed[0] or r[0] >= zeroed[0] + zeroed[1], name
    for i in range(n):
        assert inside(regions[f"table{i}"], tables) and inside(regions[f"hist{i}"], hists) and inside(regions[f"pal{i}"], pals)
        w, h = shapes[i]
        assert regions[f"out{i}"][1] == w * h * 4 and regions[f"in{i}"][1] == (w * h * 4 if inputs else 0)
    live = sorted(r for k, r in list(head.items()) + list(per_image.items()) if r[1])
    for (a, sa), (b, _) in zip(live, live[1:]):
        assert a + sa <= b, (a, sa, b)


def test_binding_tables_of_the_extension_header(tmp_path):
    """pngloss_amd.lib.QUANT_STRUCTS and QUANT_PROTOTYPES against what the compiler makes of include/pngloss_hip_quant.h, with the comparisons
    tests/test_abi.py uses for pngloss_hip.h; and the library exports both calls"""
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_quant.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.QUANT_PROTOTYPES) == ["pngloss_hip_multi_quantize_batch_host", "pngloss_hip_quantize_batch"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.QUANT_STRUCTS) == ["pngloss_hip_quant_params", "pngloss_hip_quant_report"]
    assert '#include "pngloss_hip.h"' in header
    taken = set(L.PROTOTYPES) | set(L.INDEXED_PROTOTYPES)
    assert not set(L.QUANT_PROTOTYPES) & taken and not set(L.QUANT_STRUCTS) & (set(L.STRUCTS) | set(L.INDEXED_STRUCTS))

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_quant.h"', "int main(void) {"]
    for name, cls in L.QUANT_STRUCTS.items():
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf("rounds . %d 0\\n", PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS);')
    seen = 0
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        name, field, size, offset = line.split()
        if name == "rounds":
            assert int(size) == 8 == L.QuantParams().rounds
            continue
        cls = L.QUANT_STRUCTS[name]
        mine = (C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        assert mine == (int(size), int(offset)), (name, field)
        seen += 1
    assert seen == 2 + len(L.QuantParams._fields_) + len(L.QuantReport._fields_)
    assert [f for f, _ in L.QuantReport._fields_] == ["status", "colors_in", "entries", "exact", "palette", "distortion"]
    assert C.sizeof(L.QuantReport) == 16 + 1024 + C.sizeof(L.Distortion) and C.sizeof(L.QuantParams) == 8

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_quant.h"
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
    assert declared["pngloss_hip_quantize_batch"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"]
    assert declared["pngloss_hip_multi_quantize_batch_host"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr"]
    assert prototype_differences(L.QUANT_PROTOTYPES, declared) == []
    for fn in functions:
        assert getattr(P.hip_lib(), fn).argtypes == L.QUANT_PROTOTYPES[fn][1]
    # the Makefile rebuilds the library when the header changes
    assert "../../include/pngloss_hip_quant.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_argument_checks_need_no_device():
    """NULL arguments, N outside 2..256 and R above 64 are refused before any device work: with no context at all the answer is the same code"""
    lib = P.hip_lib()
    rep = (L.QuantReport * 1)()
    descs = (L.ImageDesc * 1)(L.ImageDesc(None, None, 4, 4))
    hosts = (L.HostImage * 1)(L.HostImage(None, None, 4, 4))
    good = L.QuantParams(16, 8)
    assert lib.pngloss_hip_quantize_batch(None, descs, 1, C.byref(good), rep, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host(None, hosts, 1, C.byref(good), rep) == INVALID
    assert lib.pngloss_hip_quantize_batch(None, None, 0, None, None, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host(None, None, 0, None, None) == INVALID
    assert (L.QuantParams().max_colors, L.QuantParams().rounds) == (256, 8)


def test_restatement_arithmetic():
    assert int(Q.bin_of(np.array([0x80123456], np.uint32))[0]) == 0x5 | 0x3 << 4 | 0x1 << 8 | 0x8 << 12
    assert Q._mean(3, 2) == 2 and Q._mean(5, 4) == 1 and Q._mean(255 * 7, 7) == 255           # (2s + n) // 2n: halves go up
    assert list(Q.nearest(np.array([0xFF000030], np.uint32), [0xFF000018, 0xFF000048])) == [0]  # a tie: the lowest entry
    r = Q.restate(np.zeros((0, 0, 4), np.uint8), 16)
    assert (r["colors_in"], r["entries"], r["exact"], r["palette"]) == (0, 0, 1, []) and r["distortion"]["pixels"] == 0


# ---- the switch ----

@pytest.fixture(scope="module")
def colors_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cli_colors") / "cli_colors_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_colors_host.c"),
                    os.path.join(CLI, "cli_options.c"), os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)
    return exe


def _cli(exe, args, cwd):
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


def test_colors_parses_and_implies_indexed_at_strength_0(colors_host, tmp_path):
    base = dict(have_colors="1", colors="16", have_strength="0", strength="0", indexed="1", gpu_deflate="1", distortion="0", verbose="0", search="none")
    for args, differs in ((["--colors", "16", "x.png"], {}), (["--colors", "2", "x.png"], dict(colors="2")), (["--colors", "256", "x.png"], dict(colors="256")),
                          (["--colors", "16", "-s", "0", "x.png"], dict(have_strength="1")), (["-s", "0", "--colors", "16", "--indexed", "--gpu-deflate", "x.png"], dict(have_strength="1")),
                          (["--colors", "16", "--distortion", "-v", "x.png"], dict(distortion="1", verbose="1"))):
        r = _cli(colors_host, args, tmp_path)
        assert r.returncode == 0 and r.stderr == "" and _fields(r.stdout) == dict(base, **differs), (args, r.stderr)
    r = _cli(colors_host, ["x.png"], tmp_path)       # without the switch nothing of it shows
    assert _fields(r.stdout) == dict(have_colors="0", colors="0", have_strength="0", strength="19", indexed="0", gpu_deflate="0", distortion="0", verbose="0", search="none")


def test_colors_refusals(colors_host, tmp_path):
    x = ["x.png"]
    rng = "Must specify a number of colours in the range 2-256.\n"
    strength = "--colors cannot be combined with a strength above 0: the palette is the lossy step.\n"
    other = "--colors cannot be combined with --target-size, --target-psnr, --target-ssim, --max-error, --ssim or --visible.\n"
    seen = {("--colors", "x"): "--colors requires a numeric argument\n", ("--colors", "1"): rng, ("--colors", "0"): rng, ("--colors", "257"): rng,
            ("--colors", "16", "-s", "19"): strength, ("-s", "1", "--colors", "16"): strength,
            ("--colors", "16", "--target-size", "10k"): other, ("--colors", "16", "--target-psnr", "40"): other, ("--colors", "16", "--target-ssim", "0.9"): other,
            ("--colors", "16", "--max-error", "3"): other, ("--colors", "16", "--ssim"): other, ("--colors", "16", "--visible", "--distortion"): other}
    for args, message in seen.items():
        r = _cli(colors_host, list(args) + x, tmp_path)
        assert (r.returncode, r.stderr, r.stdout) == (INVALID, message, ""), args
    assert not os.listdir(tmp_path)


def test_colors_is_absent_from_the_usage_text_which_stays_as_recorded():
    import json
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        rec = {tuple(v["args"]): v for v in json.load(fh)["vectors"]}
    text = open(os.path.join(CLI, "cli_options.c")).read()
    usage = "".join(re.findall(r'^    "((?:[^"\\]|\\.)*)"', text[text.index("const char cli_usage_text[]"):text.index("enum {")], flags=re.M))
    usage = usage.encode().decode("unicode_escape")
    assert "--colors" not in usage and usage in rec[("--help",)]["stdout"]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "--colors" in open(os.path.join(U.ROOT, doc)).read(), doc


def test_verbose_line(colors_host):
    line = lambda *a: subprocess.run([colors_host, "report"] + [str(v) for v in a], capture_output=True, text=True, check=True).stdout
    assert line(257, 16, 0) == "  colors: more than 256 in the input, 16 palette entries\n"
    assert line(194, 194, 1) == "  colors: 194 in the input, 194 palette entries, exact (no pixel changed)\n"
    assert line(200, 16, 0) == "  colors: 200 in the input, 16 palette entries\n"


# ---- quality ----

def _pillow(img, n):
    from PIL import Image
    opaque = bool((img[..., 3] == 255).all())
    im = Image.fromarray(img, "RGBA")
    q = (im.convert("RGB") if opaque else im).quantize(colors=n, method=0 if opaque else 2, dither=Image.Dither.NONE)
    return np.asarray(q.convert("RGBA"))


@pytest.mark.parametrize("name,n", [("rose", 16), ("rose", 256), ("tux", 16), ("tux", 256)])
def test_quality_is_not_below_pillows(name, n):
    """four-channel PSNR over all pixels, R = 8, Pillow without dithering (method 0 for opaque images, 2 for images with alpha).  No margin: the
    slack measured when the definitions were drafted was 1.6 to 6.1 dB"""
    img = U.load_npz("suite_inputs.npz")[name]
    mine = Q.restate(img, n, 8)
    theirs = _pillow(img, n)
    a, b = Q.psnr4(img, mine["pixels"]), Q.psnr4(img, theirs)
    print(name, n, "restatement %.2f dB" % a, "Pillow %.2f dB" % b)
    assert a >= b
    if (name, n) == ("tux", 256):
        assert mine["exact"] == 1 and mine["colors_in"] == 194 and np.array_equal(mine["pixels"], img)

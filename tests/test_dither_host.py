"""CPU tests of the quantiser's error diffusion (no GPU): the core of pngloss_amd/csrc/pl_dither_core.h run in the kernel's own order under the
sanitizers against the raster-order restatement of tests/util_dither.py; the schedule arithmetic, exhaustively; the layout of the job table and the
error lines; the binding tables against the compiler's view of include/pngloss_hip_dither.h; the argument checks that need no device; the switch
--dither; and what the rule is for, on the restatement alone."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_dither as F
from tests import util_quant as Q

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
INVALID = L.PNGLOSS_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return F.build_dither_host(tmp_path_factory.mktemp("dither_host"))


def test_restated_constants_are_the_headers(exe):
    assert [int(v) for v in F.run_host(exe, ["constants"]).split()] == [F.LANES, F.WAVES, F.BAND, F.K, F.LAG, F.RING]
    assert F.BAND == F.LANES * F.WAVES and 4 <= F.WAVES <= 16 and F.LAG * F.K >= 2 * (F.LANES - 1) + 1 + F.K - 1
    sizes = [(1, 1), (1, F.BAND + 1), (2 * F.K + 1, 1), (F.K + 1, 65), (3, 2 * F.BAND + 1), (3 * F.K + 5, F.BAND + 2), (1920, 1080), (4096, 4096), (0, 5), (5, 0)]
    got = [int(v) for v in F.run_host(exe, ["barriers"] + [str(v) for s in sizes for v in s]).split()]
    assert got == [F.barriers(w, h) for w, h in sizes]
    assert F.barriers(1, 1) == 2 and F.barriers(F.K + 1, 65) == 3 + F.LAG


def test_core_in_the_kernels_order_equals_the_restatement(exe, tmp_path):
    """every shape of the device tests, the waves of an epoch ascending and descending: they run concurrently on the device, so neither order may matter"""
    shapes = F.shapes()
    cases, want = [], {}
    for name, (img, n, rounds) in shapes.items():
        pal = F.final_palette(img, n, rounds)
        want[name] = F.diffuse(img, pal)
        cases += [(img, pal, 0), (img, pal, 1)]
    got = F.run_dither_host(exe, tmp_path, cases)
    for k, g in enumerate(got):
        name = list(shapes)[k // 2]
        img = shapes[name][0]
        assert np.array_equal(g["pixels"], want[name]), (name, k % 2)
        assert g["barriers"] == F.barriers(img.shape[1], img.shape[0]), name
    clamp = got[2 * list(shapes).index("clamp")]
    assert clamp["a_min"] < 0 and clamp["a_max"] > 255


def test_schedule_arithmetic_exhaustively(exe):
    """every width in 1 .. 3K+2 and height in 1 .. 2*band+2, as the columns each lane covers in each epoch: every pixel once and in order, never
    before (y, x-1) and (y-1, x+1) -- across waves only what the wave above had finished when the epoch began counts --, the same barriers for
    every wave, and no ring slot or error-line entry written before its reader has passed it"""
    w, h = 3 * F.K + 2, 2 * F.BAND + 2
    out = F.run_host(exe, ["sched", str(w), str(h)]).split()
    assert out[0] == "ok" and int(out[1]) == w * h, out
    assert int(out[2]) >= w * (F.BAND + 2)                          # bands walked: every row count alone, and the full band in each of its places


def test_layout_of_the_job_table_and_the_error_lines(exe):
    widths = [70, 0, 1, 257, 5, 4096]
    base, job_bytes = 1000, 48
    out = F.run_host(exe, ["layout", str(base), str(job_bytes)] + [str(w) for w in widths])
    regions = {name: (int(at), int(size)) for name, at, size in (line.split() for line in out.splitlines())}
    total = regions.pop("total")[1]
    lines = regions.pop("lines")
    assert regions["jobs"][1] == job_bytes * len(widths) and regions["jobs"][0] >= base
    for name, (at, size) in regions.items():
        assert at % 256 == 0 and at >= base and at + size <= total, name
    for i, w in enumerate(widths):
        at, size = regions[f"line{i}"]
        assert size == 8 * w and lines[0] <= at and at + size <= lines[0] + lines[1]      # W entries of four 16-bit errors: the widest image's too
    assert regions[f"line{widths.index(max(widths))}"][1] == 8 * max(widths)
    live = sorted(r for r in regions.values() if r[1])
    for (a, sa), (b, _) in zip(live, live[1:]):
        assert a + sa <= b
    # the quantiser's own layout function and job stay as they are: the dither pass has its own, behind it
    text = open(os.path.join(CSRC, "pl_layout.h")).read()
    assert "inline PlDitherLayout pl_dither_layout(" in text and "inline PlQuantLayout pl_quant_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs, size_t index_job_bytes," in text


def test_binding_tables_of_the_dither_header(tmp_path):
    """pngloss_amd.lib.DITHER_STRUCTS and DITHER_PROTOTYPES against what the compiler makes of include/pngloss_hip_dither.h"""
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_dither.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.DITHER_PROTOTYPES) == ["pngloss_hip_multi_quantize_batch_host2", "pngloss_hip_quantize_batch2"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.DITHER_STRUCTS) == ["pngloss_hip_quant_params2"]
    assert '#include "pngloss_hip_quant.h"' in header
    taken = set(L.PROTOTYPES) | set(L.INDEXED_PROTOTYPES) | set(L.QUANT_PROTOTYPES)
    assert not set(L.DITHER_PROTOTYPES) & taken and not set(L.DITHER_STRUCTS) & (set(L.STRUCTS) | set(L.INDEXED_STRUCTS) | set(L.QUANT_STRUCTS))

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_dither.h"', "int main(void) {"]
    for name, cls in L.DITHER_STRUCTS.items():
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf("dither . %d %d\\n", PNGLOSS_HIP_DITHER_NONE, PNGLOSS_HIP_DITHER_FLOYD_STEINBERG);')
    seen = 0
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        name, field, size, offset = line.split()
        if name == "dither":
            assert (int(size), int(offset)) == (0, 1) == (L.DITHER_NONE, L.DITHER_FLOYD_STEINBERG)
            continue
        cls = L.DITHER_STRUCTS[name]
        mine = (C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        assert mine == (int(size), int(offset)), (name, field)
        seen += 1
    assert seen == 1 + len(L.QuantParams2._fields_)
    assert [f for f, _ in L.QuantParams2._fields_] == ["max_colors", "rounds", "dither", "reserved"] and C.sizeof(L.QuantParams2) == 16
    p = L.QuantParams2()
    assert (p.max_colors, p.rounds, p.dither, p.reserved) == (256, 8, 0, 0)

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_dither.h"
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
    assert declared["pngloss_hip_quantize_batch2"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"]
    assert declared["pngloss_hip_multi_quantize_batch_host2"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr"]
    assert prototype_differences(L.DITHER_PROTOTYPES, declared) == []
    for fn in functions:                                             # the library exports both, and hip_lib() has given them their prototypes
        assert getattr(P.hip_lib(), fn).argtypes == L.DITHER_PROTOTYPES[fn][1]
    assert "../../include/pngloss_hip_dither.h" in open(os.path.join(CSRC, "Makefile")).read()
    # the quantiser's own header points here and is otherwise what it was
    quant = open(os.path.join(include, "pngloss_hip_quant.h")).read()
    assert "No dithering" not in quant and "pngloss_hip_dither.h" in quant


def test_argument_checks_need_no_device():
    """dither above 1, reserved not 0 and NULLs are refused before any device work: with no context at all the answer is the same code"""
    lib = P.hip_lib()
    rep = (L.QuantReport * 1)()
    descs = (L.ImageDesc * 1)(L.ImageDesc(None, None, 4, 4))
    hosts = (L.HostImage * 1)(L.HostImage(None, None, 4, 4))
    for params in (L.QuantParams2(16, 8, 1), L.QuantParams2(16, 8, 0), L.QuantParams2(16, 8, 2), L.QuantParams2(16, 8, 1, 1), L.QuantParams2(1, 8, 1), L.QuantParams2(16, 65, 1)):
        assert lib.pngloss_hip_quantize_batch2(None, descs, 1, C.byref(params), rep, None) == INVALID
        assert lib.pngloss_hip_multi_quantize_batch_host2(None, hosts, 1, C.byref(params), rep) == INVALID
    assert lib.pngloss_hip_quantize_batch2(None, None, 0, None, None, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host2(None, None, 0, None, None) == INVALID
    # the refusals of the parameters themselves are in the one check both forms ask
    host = open(os.path.join(CSRC, "pl_host_quant.hip")).read()
    assert "if (params->dither > PNGLOSS_HIP_DITHER_FLOYD_STEINBERG || params->reserved) return PNGLOSS_INVALID_ARGUMENT;" in host
    assert host.count("check_quant_params(params)") == 2


# ---- the switch ----

@pytest.fixture(scope="module")
def dither_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cli_dither") / "cli_dither_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_dither_host.c"),
                    os.path.join(CLI, "cli_options.c"), os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)
    return exe


def _cli(exe, args, cwd):
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


def test_dither_parses_with_colors(dither_host, tmp_path):
    base = dict(dither="1", have_colors="1", colors="16", have_strength="0", strength="0", indexed="1", gpu_deflate="1", distortion="0", verbose="0")
    for args, differs in ((["--colors", "16", "--dither", "x.png"], {}), (["--dither", "--colors", "2", "x.png"], dict(colors="2")),
                          (["--colors", "16", "--dither", "--distortion", "-v", "x.png"], dict(distortion="1", verbose="1")),
                          (["--colors", "16", "x.png"], dict(dither="0"))):
        r = _cli(dither_host, args, tmp_path)
        assert r.returncode == 0 and r.stderr == "" and _fields(r.stdout) == dict(base, **differs), (args, r.stderr)


def test_dither_is_refused_without_colors(dither_host, tmp_path):
    for args in (["--dither", "x.png"], ["--dither", "-s", "0", "--indexed", "x.png"], ["-v", "--dither", "-o", "y.png", "x.png"]):
        r = _cli(dither_host, args, tmp_path)
        assert (r.returncode, r.stderr, r.stdout) == (INVALID, "--dither requires --colors.\n", ""), args
    r = _cli(dither_host, ["--dither=1", "--colors", "16", "x.png"], tmp_path)      # it takes no argument
    assert r.returncode == INVALID and r.stdout == ""
    assert not os.listdir(tmp_path)


def test_dither_is_absent_from_the_usage_text_which_stays_as_recorded(dither_host):
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        rec = {tuple(v["args"]): v for v in json.load(fh)["vectors"]}
    usage = subprocess.run([dither_host, "usage"], capture_output=True, text=True, check=True).stdout
    assert "--dither" not in usage and "--colors" not in usage and usage and usage in rec[("--help",)]["stdout"]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "--dither" in open(os.path.join(U.ROOT, doc)).read(), doc


def test_verbose_lines(dither_host):
    line = lambda *a: subprocess.run([dither_host, "report"] + [str(v) for v in a], capture_output=True, text=True, check=True).stdout
    assert line(257, 16, 0) == "  colors: more than 256 in the input, 16 palette entries\n  dither: Floyd-Steinberg\n"
    assert line(200, 16, 0) == "  colors: 200 in the input, 16 palette entries\n  dither: Floyd-Steinberg\n"
    assert line(194, 194, 1) == "  colors: 194 in the input, 194 palette entries, exact (no pixel changed)\n"      # an exact file is never dithered


# ---- what the rule is for (the restatement alone) ----

@pytest.mark.parametrize("name", ["gradient", "rose"])
def test_block_means_come_closer_to_the_input(name):
    """RMS over the 8x8 block means against the input, R = 8: smaller dithered than nearest-entry, at every N"""
    img = F.gradient(96, 64) if name == "gradient" else U.load_npz("suite_inputs.npz")["rose"]
    for n in (4, 16, 64):
        plain, dithered = Q.restate(img, n, 8), F.restate(img, n, 8)
        a, b = F.block_rms(img, plain["pixels"]), F.block_rms(img, dithered["pixels"])
        print(name, n, "nearest entry %.2f" % a, "dithered %.2f" % b, "entries", plain["entries"], dithered["entries"])
        assert b < a
        assert dithered["exact"] == 0 and dithered["entries"] <= n


def test_the_clamp_case_saturates_at_both_ends():
    img, n, rounds = F.shapes()["clamp"]
    stats = {}
    r = F.restate(img, n, rounds, stats)
    assert stats["a_min"] < 0 and stats["a_max"] > 255 and r["exact"] == 0
    assert -255 <= stats["a_min"] and stats["a_max"] <= 510


def test_restatement_arithmetic():
    """one row, one column and the corner by hand; an exact image is not dithered"""
    pal = [0xFF000000, 0xFF0000FF]                              # red 0 and 255
    row = Q.from_words(np.array([0xFF000064, 0xFF000064, 0xFF000064], np.uint32), 3, 1)      # red 100: e = 100, then a = 100 + (700 + 8 >> 4) = 144 -> 255, e = -111
    out = Q.words(F.diffuse(row, pal))
    assert list(out) == [0xFF000000, 0xFF0000FF, 0xFF000000] and (700 + 8) >> 4 == 44 and 100 + ((7 * -111 + 8) >> 4) == 51
    col = Q.from_words(np.array([0xFF000064, 0xFF000064], np.uint32), 1, 2)                   # below: only the 5/16 term, a = 100 + (500 + 8 >> 4) = 131 -> 255
    assert list(Q.words(F.diffuse(col, pal))) == [0xFF000000, 0xFF0000FF] and 100 + ((500 + 8) >> 4) == 131
    assert (-9) >> 4 == -1 and (-8 + 8) >> 4 == 0 and (7 * -255 - 255 + 5 * -255 + 3 * -255 + 8) >> 4 == -255      # the shift rounds down
    two = Q.from_words(np.array([0xFF102030, 0xFFE0D0C0], np.uint32)[[0, 1, 1, 0]], 2, 2)
    r = F.restate(two, 2, 8)
    assert r["exact"] == 1 and np.array_equal(r["pixels"], two)

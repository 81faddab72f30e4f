"""CPU tests of the quantiser's colour-count search (no GPU): the rule of pngloss_amd/csrc/pl_colors.h against its restatement in Python over every
M, every monotone acceptance threshold and seeded non-monotone tables; the lane loop of pl_quant_measure (pl_quant_measure_core.h) under the
sanitizers against numpy's record of the restated remap; the binding tables against the compiler's view of include/pngloss_hip_quant_target.h; the
argument checks that need no device; the switches --colors-psnr and --colors-max-error; and the procedure end to end on the restatement alone."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_distort as D
from tests import util_dither as F
from tests import util_quant as Q
from tests import util_quant_target as T

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
INVALID = L.PNGLOSS_INVALID_ARGUMENT


# ---- the rule ----

@pytest.fixture(scope="module")
def colors_exe(tmp_path_factory):
    return T.build_colors_host(tmp_path_factory.mktemp("colors_host"))


def _tables():
    """(M, table): table[N] is whether a probe at N is accepted.  Every M in 2 .. 256 with every monotone threshold (accepted from t on; t = M + 1:
    nothing is), and 300 seeded tables with no order at all"""
    out = []
    for m in range(2, 257):
        for t in range(2, m + 2):
            out.append((m, [n >= t for n in range(m + 1)]))
    rng = np.random.default_rng(53)
    for k in range(300):
        m = int(rng.integers(2, 257))
        out.append((m, [bool(v) for v in rng.random(m + 1) < (0.2, 0.5, 0.8)[k % 3]]))
    return out


def test_search_rule_against_the_restatement(colors_exe, tmp_path):
    tables = _tables()
    lines = T.run_colors_host(colors_exe, tmp_path, ["S %d %s" % (m, "".join("01"[v] for v in table)) for m, table in tables])
    wandering = 0
    for (m, table), line in zip(tables, lines):
        got = [int(v) for v in line.split()]
        want = T.search(lambda n: table[n], m)
        assert got[:5] == [want["colors"], want["reached"], want["probes"], T.probe_bound(m), want["accepted_mask"]] and got[5:] == want["probed"], (m, line)
        assert want["probes"] <= T.probe_bound(m) <= T.MAX_PROBES and want["probed"][0] == m and all(2 <= n <= m for n in want["probed"])
        assert want["reached"] == int(table[m]) and (want["reached"] or want["colors"] == m)
        if m == 2:
            assert want["probes"] == 1 and want["colors"] == 2
        passing = [n for n in range(2, m + 1) if table[n]]
        if want["reached"]:
            assert table[want["colors"]]
            wandering += want["colors"] != passing[0]
        if sorted(table[2:]) == table[2:]:                          # monotone: the procedure finds the smallest N that passes
            assert want["colors"] == (passing[0] if passing else m)
    assert wandering > 50                                            # the seeded tables do tell the procedure from "the smallest N that passes"
    assert T.probe_bound(256) == 9 and T.probe_bound(2) == 1 and T.probe_bound(3) == 2 and T.probe_bound(4) == 3


def test_the_same_program_without_the_sanitizers_agrees(colors_exe, tmp_path):
    """(the sanitized binary is a stand-alone program: it needs nothing preloaded.  Built plainly and optimised, the header answers the same)"""
    exe = str(tmp_path / "colors_host_plain")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(U.ROOT, "tests", "c", "colors_host.cpp")], check=True, capture_output=True)
    commands = ["S %d %s" % (m, "".join("01"[v] for v in table)) for m, table in _tables()[::7]]
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(commands) + "\n")
    plain = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert plain == T.run_colors_host(colors_exe, tmp_path, commands)


def test_probes_without_device_work_and_the_round(colors_exe, tmp_path):
    cases = [(256, 0, 0), (256, 100, 194), (256, 100, 257), (16, 100, 16), (16, 100, 17), (2, 100, 2), (2, 100, 3), (256, 100, 1)]
    lines = T.run_colors_host(colors_exe, tmp_path, ["E %d %d %d" % c for c in cases] + ["G 256 -1 128 2 -1", "G -1", "G"])
    for (m, pixels, colors_in), line in zip(cases, lines):
        stepped, done, chosen, reached, nxt = (int(v) for v in line.split())
        # restated: exact probes are accepted one after the other until one needs the device
        probed = []

        class NeedsDevice(Exception):
            pass

        def accepted(n):
            if pixels and n < colors_in:
                raise NeedsDevice(n)
            probed.append(n)
            return True
        try:
            want = T.search(accepted, m)
            assert (stepped, done, chosen, reached) == (want["probes"], 1, 2, 1), (m, pixels, colors_in)
        except NeedsDevice as stop:
            assert (stepped, done, nxt) == (len(probed), 0, stop.args[0]), (m, pixels, colors_in)
    assert lines[len(cases):] == ["0:256 2:128 3:2", "", ""]


def test_acceptance_and_the_target_check(colors_exe, tmp_path):
    rec = dict(pixels=1000, changed_pixels=900, sq_err=[40000, 30000, 20000, 10000], max_abs=[9, 30, 7, 5])
    psnr = D.py_psnr_db(rec, 0xF)
    assert math.isclose(psnr, 10 * math.log10(255 * 255 * 4000 / 100000))
    zero = dict(pixels=1000, changed_pixels=0, sq_err=[0] * 4, max_abs=[0] * 4)
    empty = dict(pixels=0, changed_pixels=0, sq_err=[5] * 4, max_abs=[200] * 4)
    line = lambda t, r: "A %s %d %d %d %s %s" % (T.double_bits(t[0]), t[1], r["pixels"], r["changed_pixels"], " ".join(map(str, r["sq_err"])), " ".join(map(str, r["max_abs"])))
    targets = [(psnr - 1e-9, 0), (psnr + 1e-9, 0), (psnr, 0), (0.0, 30), (0.0, 29), (psnr - 1, 29), (psnr + 1, 30), (psnr - 1, 30), (math.inf, 0), (math.inf, 1)]
    cases = [(t, r) for t in targets for r in (rec, zero, empty)]
    got = T.run_colors_host(colors_exe, tmp_path, [line(t, r) for t, r in cases])
    assert [int(v) for v in got] == [int(T.accepts(r, *t)) for t, r in cases]
    assert [int(v) for v in got[:3]] == [1, 1, 1] and [int(v) for v in got[3:6]] == [0, 1, 1] and int(got[4 * 3]) == 0 and int(got[8 * 3 + 1]) == 1
    checks = {("null",): INVALID, (T.double_bits(30.0), 0, 0): 0, (T.double_bits(0.0), 60, 0): 0, (T.double_bits(30.0), 255, 0): 0, (T.double_bits(math.inf), 0, 0): 0,
              (T.double_bits(0.0), 0, 0): INVALID, (T.double_bits(math.nan), 0, 0): INVALID, (T.double_bits(math.nan), 3, 0): INVALID,
              (T.double_bits(-1.0), 0, 0): INVALID, (T.double_bits(-0.5), 9, 0): INVALID, (T.double_bits(30.0), 256, 0): INVALID, (T.double_bits(30.0), 0, 1): INVALID}
    got = T.run_colors_host(colors_exe, tmp_path, ["C " + " ".join(str(v) for v in c) for c in checks])
    assert [int(v) for v in got] == list(checks.values())


# ---- the measuring body ----

def _measure_cases():
    """name -> (image, final palette): the shapes of the issue's list, and one lane taken past what its 32-bit sums hold"""
    shapes = Q.shapes()
    rose = shapes["rose_16"][0]
    picked = {name: shapes[name] for name in ("1x1", "1x7", "5x1", "three_colours_one_equidistant", "noise_257x33")}
    for n in (3, 5, 7, 16, 255):
        picked[f"rose_{n}"] = (rose, n, 2 if n != 16 else 8)
    out = {}
    for name, (img, n, rounds) in picked.items():
        pal = F.final_palette(img, n, rounds)
        if pal is None:                                             # an exact image: its own colours are a palette that changes nothing
            pal = [int(x) for x in np.unique(Q.words(img))]
        out[name] = (img, pal, Q.restate(img, n, rounds)["pixels"])
    return out


def test_measuring_body_equals_numpy_on_the_restated_remap(tmp_path):
    exe = T.build_measure_host(tmp_path)
    flush, lane_max, wg_pixels, quad = T.measure_constants(exe)
    assert flush + quad - 1 <= lane_max == 0xFFFFFFFF // (255 * 255) and wg_pixels // 256 > flush       # a lane of the kernel can pass its flush: it has to empty its sums
    cases, want = [], []
    for name, (img, pal, remapped) in _measure_cases().items():
        rec = D.np_distortion(img, remapped)
        assert name in ("1x1",) or rec["changed_pixels"] > 0, name
        for blocks, lanes, team, offset in ((1, 1, 0, 0), (2, 4, 0, 0), (3, 4, 1, 0), (1, 64, 0, 0), (2, 4, 0, 1), (3, 4, 1, 1)):
            cases.append((img, pal, blocks, lanes, team, offset))
            want.append((name, rec))
    # one lane alone over 70 000 white pixels against two entries near black: 70 000 * 254^2 is past 2^32, and so is a lane's share that is not flushed
    white = Q.from_words(np.full(70000, 0xFFFFFFFF, np.uint32), 70000, 1)
    pal = [0x00000000, 0x00000001]
    rec = D.np_distortion(white, Q.from_words(np.full(70000, 0x00000001, np.uint32), 70000, 1))
    assert rec["sq_err"][0] > 1 << 32 and 70000 > lane_max
    for blocks, lanes, team, offset in ((1, 1, 0, 0), (1, 1, 0, 1), (2, 2, 1, 0)):
        cases.append((white, pal, blocks, lanes, team, offset))
        want.append(("lane_past_its_sums", rec))
    got = T.run_measure_host(exe, tmp_path, cases)
    for g, (name, rec), case in zip(got, want, cases):
        assert g == {k: rec[k] for k in ("changed_pixels", "sq_err", "max_abs")}, (name, case[2:])


def test_the_kernel_runs_the_core_and_states_its_lane_bound():
    text = open(os.path.join(CSRC, "pl_quant.hip")).read()
    assert "plq_measure_lane(pal2, entries, j.img, n, blockIdx.x, gridDim.x, threadIdx.x, kThreads)" in text and "static_assert(PLQ_WG_PIXELS / kThreads" in text
    core = open(os.path.join(CSRC, "pl_quant_measure_core.h")).read()
    assert "pld_flush(s, l)" in core and "plq_search_quad(pal2, entries, w, m, best)" in core and "static_assert(PLD_FLUSH_PIXELS + PLQ_QUAD - 1 <= PLD_LANE_PIXELS_MAX" in core
    body = text[text.index("void pl_quant_measure("):text.index("void pl_quant_update(")]
    assert "j.out" not in body                                       # it stores no pixel


# ---- the binding ----

def test_binding_tables_of_the_target_header(tmp_path):
    """pngloss_amd.lib.QUANT_TARGET_STRUCTS and QUANT_TARGET_PROTOTYPES against what the compiler makes of include/pngloss_hip_quant_target.h"""
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_quant_target.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.QUANT_TARGET_PROTOTYPES) == ["pngloss_hip_multi_quantize_batch_host_target", "pngloss_hip_quantize_batch_target"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.QUANT_TARGET_STRUCTS) == ["pngloss_hip_quant_target", "pngloss_hip_quant_target_report"]
    assert '#include "pngloss_hip_dither.h"' in header
    taken = set(L.PROTOTYPES) | set(L.INDEXED_PROTOTYPES) | set(L.QUANT_PROTOTYPES) | set(L.DITHER_PROTOTYPES)
    structs = set(L.STRUCTS) | set(L.INDEXED_STRUCTS) | set(L.QUANT_STRUCTS) | set(L.DITHER_STRUCTS)
    assert not set(L.QUANT_TARGET_PROTOTYPES) & taken and not set(L.QUANT_TARGET_STRUCTS) & structs

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_quant_target.h"', "int main(void) {"]
    for name, cls in L.QUANT_TARGET_STRUCTS.items():
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf("probes . %d 0\\n", PNGLOSS_HIP_QUANT_TARGET_MAX_PROBES);')
    seen = 0
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        name, field, size, offset = line.split()
        if name == "probes":
            assert int(size) == 12 == T.MAX_PROBES
            continue
        cls = L.QUANT_TARGET_STRUCTS[name]
        mine = (C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        assert mine == (int(size), int(offset)), (name, field)
        seen += 1
    assert seen == 2 + len(L.QuantTarget._fields_) + len(L.QuantTargetReport._fields_)
    assert [f for f, _ in L.QuantTarget._fields_] == ["min_psnr_db", "max_abs_error", "reserved"] and C.sizeof(L.QuantTarget) == 16
    assert [f for f, _ in L.QuantTargetReport._fields_] == ["colors", "reached", "probes", "accepted_mask", "probed", "probe_distortion", "quant"]
    assert C.sizeof(L.QuantTargetReport) == 16 + 48 + C.sizeof(L.Distortion) + C.sizeof(L.QuantReport)
    t = L.QuantTarget()
    assert (t.min_psnr_db, t.max_abs_error, t.reserved) == (0.0, 0, 0)

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_quant_target.h"
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
    assert declared["pngloss_hip_quantize_batch_target"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr", "ptr"]
    assert declared["pngloss_hip_multi_quantize_batch_host_target"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"]
    assert prototype_differences(L.QUANT_TARGET_PROTOTYPES, declared) == []
    for fn in functions:                                             # the library exports both, and hip_lib() has given them their prototypes
        assert getattr(P.hip_lib(), fn).argtypes == L.QUANT_TARGET_PROTOTYPES[fn][1]
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "../../include/pngloss_hip_quant_target.h" in make and "pl_host_quant_target.hip" in make
    # the older tables are what they were
    assert list(L.DITHER_STRUCTS) == ["pngloss_hip_quant_params2"] and len(L.STRUCTS) == 16 and len(L.QUANT_STRUCTS) == 2 and len(L.INDEXED_STRUCTS) == 1


def test_argument_checks_need_no_device():
    """an invalid target, an invalid parameter record and NULLs are refused before any device work: with no context at all the answer is the same code"""
    lib = P.hip_lib()
    rep = (L.QuantTargetReport * 1)()
    descs = (L.ImageDesc * 1)(L.ImageDesc(None, None, 4, 4))
    hosts = (L.HostImage * 1)(L.HostImage(None, None, 4, 4))
    params = L.QuantParams2(16, 8, 0)
    both = lambda p, t: (lib.pngloss_hip_quantize_batch_target(None, descs, 1, C.byref(p) if p else None, C.byref(t) if t else None, rep, None),
                         lib.pngloss_hip_multi_quantize_batch_host_target(None, hosts, 1, C.byref(p) if p else None, C.byref(t) if t else None, rep))
    targets = [L.QuantTarget(math.nan), L.QuantTarget(-1.0), L.QuantTarget(-1.0, 5), L.QuantTarget(30.0, 256), L.QuantTarget(30.0, 0, 1), L.QuantTarget(0.0, 0),
               L.QuantTarget(30.0), L.QuantTarget(0.0, 60), L.QuantTarget(math.inf), None]
    for t in targets:
        assert both(params, t) == (INVALID, INVALID)
    for p in (L.QuantParams2(1, 8), L.QuantParams2(257, 8), L.QuantParams2(16, 65), L.QuantParams2(16, 8, 2), L.QuantParams2(16, 8, 0, 1), None):
        assert both(p, L.QuantTarget(30.0)) == (INVALID, INVALID)
    assert lib.pngloss_hip_quantize_batch_target(None, None, 0, None, None, None, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host_target(None, None, 0, None, None, None) == INVALID
    # the checks are the older calls' and pl_colors.h's, in one place for both forms, in front of everything else
    host = open(os.path.join(CSRC, "pl_host_quant_target.hip")).read()
    assert host.count("check_quant_params(params) || pl_colors_target_check(target)") == 1 and host.count("check_target_call(") == 3
    assert "deal_over_contexts(m, images, n, nullptr, nullptr, nullptr, false," in host and "forget_last_batch" not in host


# ---- the switches ----

@pytest.fixture(scope="module")
def target_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cli_colors_target") / "cli_colors_target_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_colors_target_host.c"),
                    os.path.join(CLI, "cli_options.c"), os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)
    return exe


def _cli(exe, args, cwd):
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


def test_switches_parse_with_colors(target_host, tmp_path):
    base = dict(have_colors="1", colors="256", have_colors_psnr="1", colors_psnr="30", have_colors_max_error="0", colors_max_error="0", dither="0", strength="0",
                indexed="1", gpu_deflate="1", distortion="0", verbose="0")
    for args, differs in ((["--colors", "256", "--colors-psnr", "30", "x.png"], {}),
                          (["--colors-psnr", "38.5", "--colors", "16", "x.png"], dict(colors="16", colors_psnr="38.5")),
                          (["--colors", "256", "--colors-max-error", "60", "x.png"], dict(have_colors_psnr="0", colors_psnr="0", have_colors_max_error="1", colors_max_error="60")),
                          (["--colors", "256", "--colors-psnr", "30", "--colors-max-error", "255", "--dither", "--distortion", "-v", "x.png"],
                           dict(have_colors_max_error="1", colors_max_error="255", dither="1", distortion="1", verbose="1")),
                          (["--colors", "256", "--colors-psnr", "inf", "x.png"], dict(colors_psnr="inf")),
                          (["--colors", "256", "x.png"], dict(have_colors_psnr="0", colors_psnr="0"))):
        r = _cli(target_host, args, tmp_path)
        assert r.returncode == 0 and r.stderr == "" and _fields(r.stdout) == dict(base, **differs), (args, r.stderr)


def test_refusals_and_their_order(target_host, tmp_path):
    x = ["x.png"]
    other = "--colors cannot be combined with --target-size, --target-psnr, --target-ssim, --max-error, --ssim or --visible.\n"
    seen = {("--colors-psnr", "30"): "--colors-psnr requires --colors.\n", ("--colors-max-error", "9"): "--colors-max-error requires --colors.\n",
            ("--colors-psnr", "30", "--colors-max-error", "9"): "--colors-psnr requires --colors.\n",
            ("--colors", "16", "--colors-psnr", "x"): "--colors-psnr requires a numeric argument\n",
            ("--colors", "16", "--colors-psnr", "0"): "Must specify a colour PSNR target above 0 dB.\n",
            ("--colors", "16", "--colors-psnr", "-3"): "Must specify a colour PSNR target above 0 dB.\n",
            ("--colors", "16", "--colors-psnr", "nan"): "Must specify a colour PSNR target above 0 dB.\n",
            ("--colors", "16", "--colors-max-error", "x"): "--colors-max-error requires a numeric argument\n",
            ("--colors", "16", "--colors-max-error", "0"): "Must specify a largest colour channel error in the range 1-255.\n",
            ("--colors", "16", "--colors-max-error", "256"): "Must specify a largest colour channel error in the range 1-255.\n",
            # every older rule answers first
            ("--colors", "16", "--target-psnr", "40", "--colors-psnr", "30"): other, ("--colors", "16", "--max-error", "3", "--colors-max-error", "3"): other,
            ("--colors", "1", "--colors-psnr", "x"): "Must specify a number of colours in the range 2-256.\n",
            ("--dither", "--colors-psnr", "30"): "--dither requires --colors.\n",
            ("--colors-psnr", "x", "-s", "300"): "Must specify a strength in the range 0-255.\n",
            ("--colors-psnr", "30", "--ext", "a", "-o", "b"): "--ext and --output options can't be used at the same time\n"}
    for args, message in seen.items():
        r = _cli(target_host, list(args) + x, tmp_path)
        assert (r.returncode, r.stderr, r.stdout) == (INVALID, message, ""), args
    r = _cli(target_host, ["--colors-psnr", "x"], tmp_path)          # ... the one about the files too
    assert r.stderr == "No input files specified.\n" and r.returncode != 0
    assert not os.listdir(tmp_path)


def test_usage_text_stays_as_recorded_and_names_neither_switch(target_host):
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        rec = {tuple(v["args"]): v for v in json.load(fh)["vectors"]}
    usage = subprocess.run([target_host, "usage"], capture_output=True, text=True, check=True).stdout
    assert "--colors" not in usage and usage and usage in rec[("--help",)]["stdout"]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(U.ROOT, doc)).read()
        assert "--colors-psnr" in text and "--colors-max-error" in text, doc


def test_verbose_lines(target_host):
    line = lambda *a: subprocess.run([target_host] + [str(v) for v in a], capture_output=True, text=True, check=True).stdout
    pixels = 46 * 70
    sq = round(255 * 255 * pixels * 4 / 10 ** 3.041)                # 30.41 dB over the four channels
    assert line("report", 27, 1, 9, 256, pixels, sq, 3000) == "  chosen: 27 of at most 256 colours, 30.41 dB (9 probes)\n"
    assert line("report", 256, 0, 1, 256, pixels, sq, 3000) == "  chosen: 256 of at most 256 colours, target not reached\n"
    assert line("report", 194, 1, 9, 256, pixels, 0, 0) == "  chosen: 194 of at most 256 colours, exact (9 probes)\n"
    assert line("missed", "a.png", 16) == "  warning: a.png: the colour target is not reached with 16 colours; written at 16 colours\n"


# ---- the procedure end to end, on the restatement alone ----

IMAGES = {}


def _probes(name):
    if name not in IMAGES:
        IMAGES[name] = T.Probes(U.load_npz("suite_inputs.npz")[name], 8)
    return IMAGES[name]


@pytest.mark.parametrize("name,want", [("rose", {25: 8, 30: 27, 35: 94, 38: 190}), ("tux", {25: 4, 30: 8, 35: 13, 38: 20})])
def test_chosen_colours_of_the_suite_images(name, want):
    """M = 256, R = 8; the table of the design note, derived here by the procedure over the restatement"""
    p = _probes(name)
    for db, colors in want.items():
        got = p.search(256, float(db))
        print(name, db, got["colors"], got["probed"], bin(got["accepted_mask"]), "%.3f dB" % p.psnr(got["colors"]), "margin %.2e" % p.margin(got, db))
        assert got["reached"] == 1 and got["probes"] == 9 and got["probed"][0] == 256 and got["colors"] == colors
        assert p.psnr(got["colors"]) >= db and p.margin(got, db) >= 1e-6
        assert got["quant"]["exact"] == 0 and got["quant"]["entries"] <= colors


@pytest.mark.parametrize("name,window", [("rose", (76, 80)), ("tux", (57, 60))])
def test_psnr_is_not_monotone_in_the_colour_count(name, window):
    """one more colour can lower the PSNR: that is why the chosen N is a procedure's and not "the smallest N that passes".  Over a window of N that
    holds such places (a scan of 2 .. 256 finds 9 on rose and 2 on tux; it takes a minute, so it is not repeated here)"""
    p = _probes(name)
    psnr = {n: p.psnr(n) for n in range(window[0], window[1] + 1)}
    drops = [n for n in range(window[0] + 1, window[1] + 1) if psnr[n] < psnr[n - 1]]
    print(name, "one more colour lowers the PSNR at", drops)
    assert drops
    # at a target between the two values the smallest passing N is below the drop, and N = drop itself does not pass
    n = drops[0]
    target = (psnr[n] + psnr[n - 1]) / 2
    assert psnr[n - 1] >= target > psnr[n]

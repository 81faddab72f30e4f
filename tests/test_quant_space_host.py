"""CPU tests of the quantiser's premultiplied space (no GPU; include/pngloss_hip_quant_space.h): plq_straight and the two facts exhaustively; the
Visible bodies of pl_quant_core.h, pl_quant_measure_core.h and pl_dither_core.h run under the sanitizers (tests/c/quant_space_host.cpp), with one
thread and with teams, against the restatement of tests/util_quant_space.py; the dither pass's schedule walked in both wave orders over alpha-0
pixels; what the space is for, on the restatement alone; the binding tables against the compiler's view of the header; the argument checks that
need no device; the switch --colors-visible; and the documents."""
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
from tests import util_quant_space as S
from tests import util_visible as V

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
INVALID = L.PNGLOSS_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def space_exe(tmp_path_factory):
    return S.build_host(tmp_path_factory.mktemp("quant_space_host"))


# ---- straight, and the two facts ----

def test_straight_over_every_entry_and_fact_1(space_exe, tmp_path):
    got = S.straight_host(space_exe, tmp_path)
    a, c = np.mgrid[0:256, 0:256].astype(np.int64)
    ch = np.minimum(255, (c * 255 + a // 2) // np.maximum(a, 1))
    want = np.where(a == 0, 0, ch | ch << 8 | ch << 16 | a << 24).astype(np.uint32)
    assert np.array_equal(got, want)
    assert all(S.straight(int(cc) * 0x010101 | int(aa) << 24) == int(want[aa, cc]) for aa, cc in ((0, 9), (1, 1), (1, 255), (3, 2), (128, 64), (255, 255), (254, 255)))
    # fact 1: pm(straight(e)) == e for every c' <= a -- on the harness's words, through util_visible.pm
    words = got.reshape(-1)
    back = S.words(V.pm(S.from_words(words, 256, 256))).reshape(256, 256)
    entry = (c | c << 8 | c << 16 | a << 24).astype(np.uint32)
    inside = c <= a
    assert int(inside.sum()) == 256 * 257 // 2 and np.array_equal(back[inside], entry[inside])
    assert all(S.pm_word(S.straight(int(e))) == int(e) for e in entry[inside][::97])
    # ... and outside it straight is total: the clamp holds, alpha stays
    assert (got >> 24 == a).all() and ((got & 255) <= 255).all() and (got[0] == 0).all()


def _cases():
    out = {}
    for n in (4, 16):
        out[f"crop_{n}"] = (S.crop(), n, 8, 0)
        out[f"crop_{n}_dithered"] = (S.crop(), n, 8, 1)
    out["dirty_8"] = (S.dirty(), 8, 8, 0)
    for name, (img, n, rounds) in S.small_shapes().items():
        out[name] = (img, n, rounds, 0)
        out[name + "_dithered"] = (img, n, rounds, 1)
    return out


@pytest.fixture(scope="module")
def restated():
    return {name: S.restate(img, n, rounds, dither) for name, (img, n, rounds, dither) in _cases().items()}


@pytest.mark.parametrize("threads", [1, 3, 8, 13])
def test_core_equals_restatement(space_exe, tmp_path, restated, threads):
    cases = _cases()
    got = S.run_host(space_exe, tmp_path, [(img, n, rounds, dither, threads, threads == 8) for img, n, rounds, dither in cases.values()])
    for (name, (img, n, rounds, dither)), g in zip(cases.items(), got):
        want = restated[name]
        assert np.array_equal(g["pixels"], want["pixels"]), name
        if want["exact"]:
            assert g["first"] == [] and np.array_equal(g["pixels"], img), name
            continue
        assert g["first"] == want["first"] and g["final"] == want["final"], name
        assert S.within_alpha(g["first"]) and S.within_alpha(g["final"]), name          # fact 2
        if not dither:                                                                   # the measuring lanes never make the straight word: fact 1 at work
            d = want["distortion"]
            assert g["record"] == [d["pixels"], d["changed_pixels"]] + d["sq_err"] + d["max_abs"], name
    assert restated["1x1"]["exact"] == 1 and restated["1x7"]["exact"] == 0
    # the four invisible words are one colour, the word 0, and cost no entry
    row = restated["transparent_row_r8"]["pixels"]
    assert (S.words(row).reshape(-1)[:4] == 0).all() and restated["transparent_row_r8"]["distortion"]["pixels"] == 3


def test_dither_schedule_over_a_band_boundary_with_invisible_pixels(space_exe, tmp_path):
    img = S.tall()
    want = S.restate(img, 5, 2, 1)
    got = S.run_host(space_exe, tmp_path, [(img, 5, 2, 1, 1, False), (img, 5, 2, 1, 1, True)])
    for g in got:
        assert np.array_equal(g["pixels"], want["pixels"]) and g["final"] == want["final"] and S.within_alpha(g["final"])
    # a pixel with alpha 0 takes no error in: what it becomes depends on the palette alone
    k = int(Q.nearest(np.array([0], np.uint32), np.array(want["final"], np.uint32))[0])
    assert (S.words(want["pixels"])[S.words(img) >> 24 == 0] == S.straight(want["final"][k])).all()


# ---- what it is for, on the restatement alone ----

def test_direction_on_the_restatement():
    gaps = []
    for img, counts in ((S.crop(), (4, 16, 64)), (S.dirty(), (8, 16))):
        for n in counts:
            plain, space = S.visible_psnr(img, Q.restate(img, n)["pixels"]), S.visible_psnr(img, S.restate(img, n)["pixels"])
            assert space >= plain + 1.0, (n, plain, space)
            gaps.append(round(space - plain, 1))
    assert gaps == [3.3, 2.3, 1.7, 2.1, 3.4]
    # with dithering, what the eye integrates of the premultiplied image is nearer too
    img = S.crop()
    plain, space = F.restate(img, 4)["pixels"], S.restate(img, 4, dither=1)["pixels"]
    assert F.block_rms(V.pm(img), V.pm(space)) < F.block_rms(V.pm(img), V.pm(plain))
    # and nothing is sprinkled into the transparent surround, next to an edge or not: it is one word, the straight word of the entry nearest to 0
    # (at N = 4 that entry has alpha 6)
    hidden = (img[..., 3] == 0).reshape(-1)
    assert len(np.unique(S.words(space)[hidden])) == 1


def test_search_accepts_a_record_without_visible_pixels():
    rng = np.random.default_rng(67)
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., :3] = rng.permutation(64).reshape(8, 8, 1) * 3
    want = S.Probes(img).search(16, min_psnr_db=40.0)
    assert (want["colors"], want["reached"], want["probed"], want["accepted_mask"]) == (2, 1, [16, 8, 4, 2], 0xF)
    assert want["quant"]["distortion"]["pixels"] == 0 and not want["quant"]["pixels"].any() and want["quant"]["exact"] == 0


# ---- the binding ----

def test_binding_tables_of_the_space_header(tmp_path):
    """pngloss_amd.lib.QUANT_SPACE_STRUCTS and QUANT_SPACE_PROTOTYPES against what the compiler makes of include/pngloss_hip_quant_space.h"""
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_quant_space.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.QUANT_SPACE_PROTOTYPES) == ["pngloss_hip_multi_quantize_batch_host3", "pngloss_hip_multi_quantize_batch_host_target3",
                                                             "pngloss_hip_quantize_batch3", "pngloss_hip_quantize_batch_target3"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.QUANT_SPACE_STRUCTS) == ["pngloss_hip_quant_params3"]
    assert '#include "pngloss_hip_quant_target.h"' in header
    taken = set(L.PROTOTYPES) | set(L.INDEXED_PROTOTYPES) | set(L.QUANT_PROTOTYPES) | set(L.DITHER_PROTOTYPES) | set(L.QUANT_TARGET_PROTOTYPES)
    structs = set(L.STRUCTS) | set(L.INDEXED_STRUCTS) | set(L.QUANT_STRUCTS) | set(L.DITHER_STRUCTS) | set(L.QUANT_TARGET_STRUCTS)
    assert not set(L.QUANT_SPACE_PROTOTYPES) & taken and not set(L.QUANT_SPACE_STRUCTS) & structs
    assert len(L.PROTOTYPES) == 49

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_quant_space.h"', "int main(void) {"]
    for name, cls in list(L.QUANT_SPACE_STRUCTS.items()) + [("pngloss_hip_quant_params2", L.QuantParams2)]:
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf("spaces . %d %d\\n", PNGLOSS_HIP_QUANT_SPACE_RGBA, PNGLOSS_HIP_QUANT_SPACE_VISIBLE);')
    layout = {}
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        name, field, size, offset = line.split()
        layout[(name, field)] = (int(size), int(offset))
    assert layout.pop(("spaces", ".")) == (0, 1) == (L.QUANT_SPACE_RGBA, L.QUANT_SPACE_VISIBLE)
    for (name, field), seen in layout.items():
        cls = L.QuantParams3 if name.endswith("3") else L.QuantParams2
        assert ((C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)) == seen, (name, field)
    assert [f for f, _ in L.QuantParams3._fields_] == ["max_colors", "rounds", "dither", "space"] and C.sizeof(L.QuantParams3) == 16
    # params2's layout, `reserved` named
    assert layout[("pngloss_hip_quant_params3", "space")] == layout[("pngloss_hip_quant_params2", "reserved")]
    p = L.QuantParams3()
    assert (p.max_colors, p.rounds, p.dither, p.space) == (256, 8, 0, 0)

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_quant_space.h"
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
    assert declared["pngloss_hip_quantize_batch3"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"]
    assert declared["pngloss_hip_multi_quantize_batch_host3"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr"]
    assert declared["pngloss_hip_quantize_batch_target3"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr", "ptr"]
    assert declared["pngloss_hip_multi_quantize_batch_host_target3"] == ["i32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"]
    assert prototype_differences(L.QUANT_SPACE_PROTOTYPES, declared) == []
    for fn in functions:                                             # the library exports all four, and hip_lib() has given them their prototypes
        assert getattr(P.hip_lib(), fn).argtypes == L.QUANT_SPACE_PROTOTYPES[fn][1]
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "../../include/pngloss_hip_quant_space.h" in make and "pl_host_quant_space.hip" in make


def test_argument_checks_need_no_device():
    """a space that is none, an invalid parameter record, an invalid target and NULLs are refused before any device work: with no context at all
    the answer is the same code from all four calls"""
    lib = P.hip_lib()
    rep, trep = (L.QuantReport * 1)(), (L.QuantTargetReport * 1)()
    descs = (L.ImageDesc * 1)(L.ImageDesc(None, None, 4, 4))
    hosts = (L.HostImage * 1)(L.HostImage(None, None, 4, 4))
    ref = lambda v: C.byref(v) if v else None
    four = lambda p, t: (lib.pngloss_hip_quantize_batch3(None, descs, 1, ref(p), rep, None), lib.pngloss_hip_multi_quantize_batch_host3(None, hosts, 1, ref(p), rep),
                         lib.pngloss_hip_quantize_batch_target3(None, descs, 1, ref(p), ref(t), trep, None),
                         lib.pngloss_hip_multi_quantize_batch_host_target3(None, hosts, 1, ref(p), ref(t), trep))
    for p in (L.QuantParams3(16, 8, 0, 2), L.QuantParams3(16, 8, 1, 0xFFFFFFFF), L.QuantParams3(1, 8), L.QuantParams3(257, 8), L.QuantParams3(16, 65),
              L.QuantParams3(16, 8, 2), L.QuantParams3(16, 8, 2, 1), None, L.QuantParams3(16, 8, 0, 1), L.QuantParams3(16, 8, 1, 0)):
        assert four(p, L.QuantTarget(30.0)) == (INVALID,) * 4                             # (the last two: a good record, and no context)
    for t in (L.QuantTarget(-1.0), L.QuantTarget(30.0, 256), L.QuantTarget(0.0, 0), None):
        assert four(L.QuantParams3(16, 8, 0, 1), t)[2:] == (INVALID, INVALID)
    assert lib.pngloss_hip_quantize_batch3(None, None, 0, None, None, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host3(None, None, 0, None, None) == INVALID
    assert lib.pngloss_hip_quantize_batch_target3(None, None, 0, None, None, None, None) == INVALID
    assert lib.pngloss_hip_multi_quantize_batch_host_target3(None, None, 0, None, None, None) == INVALID
    # the new entry points are a file of their own; the space is refused there, every older refusal by the older check
    space = open(os.path.join(CSRC, "pl_host_quant_space.hip")).read()
    assert "params->space > PNGLOSS_HIP_QUANT_SPACE_VISIBLE" in space and "hipLaunchKernelGGL" not in space and "PL_CHECK" not in space
    for name in ("pl_host_quant.hip", "pl_host_quant_target.hip"):
        assert "batch3" not in open(os.path.join(CSRC, name)).read() and "target3" not in open(os.path.join(CSRC, name)).read()


def test_kernels_of_the_space_are_instantiations_of_the_same_bodies():
    quant, dither = open(os.path.join(CSRC, "pl_quant.hip")).read(), open(os.path.join(CSRC, "pl_dither.hip")).read()
    for name in ("pl_quant_hist_visible", "pl_quant_assign_visible", "pl_quant_remap_visible", "pl_quant_measure_visible"):
        assert f"void {name}(" in quant, name
    assert "void pl_dither_visible(" in dither and "plf_pixel<Visible>(" in dither
    assert "assign_body<false, true>(jobs)" in quant and "assign_body<true, true>(jobs)" in quant and "hist_body<true>(jobs)" in quant
    core = open(os.path.join(CSRC, "pl_quant_core.h")).read()
    assert core.count("pld_pm(") >= 2 and "uint32_t pld_pm(" not in core            # pl_distort_core.h's, not a second one


# ---- the switch ----

@pytest.fixture(scope="module")
def visible_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cli_colors_visible") / "cli_colors_visible_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_colors_visible_host.c"),
                    os.path.join(CLI, "cli_options.c"), os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)
    return exe


def _cli(exe, args, cwd):
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


def test_switch_parses_with_colors_and_its_companions(visible_host, tmp_path):
    base = dict(colors_visible="1", visible="0", dither="0", have_colors="1", colors="16", have_colors_psnr="0", have_colors_max_error="0", strength="0", indexed="1",
                gpu_deflate="1", distortion="0", verbose="0")
    for args, differs in ((["--colors", "16", "--colors-visible", "x.png"], {}),
                          (["--colors-visible", "--colors", "16", "--dither", "x.png"], dict(dither="1")),
                          (["--colors", "256", "--colors-visible", "--colors-psnr", "35", "--colors-max-error", "40", "x.png"],
                           dict(colors="256", have_colors_psnr="1", have_colors_max_error="1")),
                          (["--colors", "16", "--colors-visible", "--dither", "--colors-psnr", "30", "--distortion", "-v", "x.png"],
                           dict(dither="1", have_colors_psnr="1", distortion="1", verbose="1")),
                          (["--colors", "16", "x.png"], dict(colors_visible="0"))):
        r = _cli(visible_host, args, tmp_path)
        assert r.returncode == 0 and r.stderr == "" and _fields(r.stdout) == dict(base, **differs), (args, r.stderr)


def test_refusals_and_their_order(visible_host, tmp_path):
    x = ["x.png"]
    other = "--colors cannot be combined with --target-size, --target-psnr, --target-ssim, --max-error, --ssim or --visible.\n"
    seen = {("--colors-visible",): "--colors-visible requires --colors.\n",
            ("--colors-visible", "--distortion"): "--colors-visible requires --colors.\n",
            # every older rule answers first, and the refusal of --visible stays word for word
            ("--colors", "16", "--colors-visible", "--visible", "--distortion"): other,
            ("--colors-visible", "--dither"): "--dither requires --colors.\n",
            ("--colors-visible", "--colors-psnr", "30"): "--colors-psnr requires --colors.\n",
            ("--colors", "1", "--colors-visible"): "Must specify a number of colours in the range 2-256.\n",
            ("--colors-visible", "-s", "300"): "Must specify a strength in the range 0-255.\n"}
    for args, message in seen.items():
        r = _cli(visible_host, list(args) + x, tmp_path)
        assert (r.returncode, r.stderr, r.stdout) == (INVALID, message, ""), args
    r = _cli(visible_host, ["--colors-visible"], tmp_path)           # ... the one about the files too
    assert r.stderr == "No input files specified.\n" and r.returncode != 0
    assert not os.listdir(tmp_path)                                   # no file was touched


def test_verbose_line_and_the_distortion_line(visible_host):
    line = lambda *a: subprocess.run([visible_host] + [str(v) for v in a], capture_output=True, text=True, check=True).stdout
    assert line("report", 257, 16, 0).splitlines()[1:] == ["  colour space: premultiplied"] and line("report", 257, 16, 0).startswith("  colors:")
    assert len(line("report", 9, 9, 1).splitlines()) == 1                                # an exact file: no space touched it
    rec = dict(pixels=3840, changed_pixels=3000, sq_err=[70000] * 4, max_abs=[41] * 4)
    assert line("distortion", 3840, 3000, 70000, 41, 1) == V.cli_lines(rec, V.NO_WINDOWS, 4)[0] + "\n"
    assert "(visible)" in line("distortion", 3840, 3000, 70000, 41, 1) and "(visible)" not in line("distortion", 3840, 3000, 70000, 41, 0)
    main = open(os.path.join(CLI, "pngloss_main.c")).read()
    assert "o->visible || o->colors_visible" in main and "pngloss_hip_multi_quantize_batch_host3(" in main and "pngloss_hip_multi_quantize_batch_host_target3(" in main


def test_switch_is_absent_from_the_usage_text_and_named_by_the_documents(visible_host):
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        rec = {tuple(v["args"]): v for v in json.load(fh)["vectors"]}
    usage = subprocess.run([visible_host, "usage"], capture_output=True, text=True, check=True).stdout
    assert "--colors" not in usage and usage and usage in rec[("--help",)]["stdout"]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "--colors-visible" in open(os.path.join(U.ROOT, doc)).read(), doc
    design = open(os.path.join(U.ROOT, "DESIGN.md")).read()
    assert "9.1e" in design and "pl_quant_remap_visible" in design and "pngloss_hip_quant_space.h" in open(os.path.join(U.ROOT, "INTEGRATION.md")).read()

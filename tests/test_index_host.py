"""CPU tests of the indexed-colour write side (no GPU): the kernels' logic (pngloss_amd/csrc/pl_index_core.h) run on the CPU under the sanitizers --
with one thread, and with a team of host threads that insert into one table concurrently -- against the numpy restatement of tests/util_index.py;
the restatement's own arithmetic; and the command line switch where no device is needed."""
import os
import subprocess

import numpy as np
import pytest

from tests import util as U
from tests import util_index as X

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
needs_cli = pytest.mark.skipif(not X.have_png, reason="libpng headers not found on this box: the command line tool is not built")


def _check_case(name, img, got):
    want = X.restate(img)
    assert min(got["count"], 257) == want["colors"], name
    if not want["eligible"]:
        assert "entries" not in got, name
        return
    h, w = img.shape[:2]
    assert got["entries"] == want["entries"] == got["count"] and got["trns_entries"] == want["trns_entries"], name
    assert np.array_equal(got["words"], want["words"]), name
    assert got["pitch"] % 16 == 0 and got["pitch"] >= w
    assert np.array_equal(got["rows"][:, :w], want["rows"]), name
    pad = (w + 3) // 4 * 4
    assert not got["rows"][:, w:pad].any(), name                      # the tail of the last dword
    assert (got["rows"][:, pad:] == 0xEE).all(), name                 # nothing is written beyond it
    assert not got["ids"].any(), name                                 # filter type "none" for every row


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return X.build_index_host(tmp_path_factory.mktemp("index_host"))


def test_core_equals_numpy_with_one_thread(exe, tmp_path):
    shapes = X.shapes()
    cases = [(img, 1) for img in shapes.values()]
    for (name, img), got in zip(shapes.items(), X.run_index_host(exe, tmp_path, cases)):
        _check_case(name, img, got)


def test_core_equals_numpy_with_a_team_that_inserts_concurrently(exe, tmp_path):
    """the same table from 3, 8 and 13 host threads: the count must stay exact when many threads insert the same colours at once"""
    shapes = X.shapes()
    cases = [(img, t) for t in (3, 8, 13) for img in shapes.values()]
    got = X.run_index_host(exe, tmp_path, cases)
    for k, g in enumerate(got):
        name = list(shapes)[k % len(shapes)]
        _check_case(name, shapes[name], g)
    # several runs of the shape built for contention: the count must come out 256 every time
    scattered = shapes["300x200_scattered_256"]
    for g in X.run_index_host(exe, tmp_path, [(scattered, 16)] * 6):
        assert g["count"] == 256 and np.array_equal(g["words"], X.restate(scattered)["words"])


def test_a_photograph_leaves_with_more_than_256(exe, tmp_path):
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 256, (64, 96, 4), dtype=np.uint8)
    for g in X.run_index_host(exe, tmp_path, [(noise, 1), (noise, 8)]):
        assert g["count"] > 256 and "entries" not in g
    # with one thread the early exit is exact: the lane stops at the quad after the 257th colour
    assert X.run_index_host(exe, tmp_path, [(noise, 1)])[0]["count"] <= 256 + 4


def test_restatement_arithmetic():
    assert X.overhead(194, 0) == 12 + 3 * 194 and X.overhead(1, 1) == 12 + 3 + 13 and X.overhead(256, 256) == 12 + 768 + 12 + 256
    # the issue's tux example: 194 colours, opaque, PLTE alone = 594 bytes
    assert X.keep_indexed(True, 12231, 29980, 194, 0) and not X.keep_indexed(False, 1, 29980, 194, 0)
    assert not X.keep_indexed(True, 100, 100 + X.overhead(5, 2), 5, 2)                 # a tie goes to truecolour
    assert X.keep_indexed(True, 100, 101 + X.overhead(5, 2), 5, 2)
    r = X.restate(X.from_words([0xFF000001, 0x00FFFFFF, 0xFF000001, 0x80000000], 2, 2))
    assert list(r["words"]) == [0x00FFFFFF, 0x80000000, 0xFF000001] and r["trns_entries"] == 2 and r["trns"] == b"\x00\x80"
    assert r["plte"] == b"\xff\xff\xff\x00\x00\x00\x01\x00\x00" and r["scanlines"] == b"\x00\x02\x00\x00\x02\x01"
    assert len({X.table_hash(w) for w in X.colliding_words(40, 5)}) == 1


def test_binding_tables_of_the_extension_header(tmp_path):
    """pngloss_amd.lib.INDEXED_STRUCTS and INDEXED_PROTOTYPES against what the compiler makes of include/pngloss_hip_indexed.h -- sizeof, size and
    offset of every field; return and argument classes of every function -- with the comparisons tests/test_abi.py uses for pngloss_hip.h"""
    import re
    from pngloss_amd import lib as L
    from tests.test_abi import prototype_differences
    include = os.path.join(U.ROOT, "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "pngloss_hip_indexed.h")).read(), flags=re.S)
    functions = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)) - {"defined"})
    assert functions == sorted(L.INDEXED_PROTOTYPES) == ["pngloss_hip_last_palette", "pngloss_hip_multi_last_palette"]
    assert re.findall(r"\}\s*(\w+)\s*;", header) == list(L.INDEXED_STRUCTS) == ["pngloss_hip_palette"]
    assert not set(L.INDEXED_PROTOTYPES) & set(L.PROTOTYPES) and not set(L.INDEXED_STRUCTS) & set(L.STRUCTS)

    def run(name, text, compiler):
        src = tmp_path / name
        src.write_text(text)
        subprocess.run(compiler + ["-I", include, "-o", str(src) + ".out", str(src)], check=True, capture_output=True)
        return subprocess.run([str(src) + ".out"], capture_output=True, text=True, check=True).stdout

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip_indexed.h"', "int main(void) {"]
    for name, cls in L.INDEXED_STRUCTS.items():
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f, _ in cls._fields_]
    seen = 0
    for line in run("layout.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11", "-Wall", "-Werror"]).splitlines():
        name, field, size, offset = line.split()
        cls = L.INDEXED_STRUCTS[name]
        mine = (L.C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        assert mine == (int(size), int(offset)), (name, field)
        seen += 1
    assert seen == 1 + len(L.Palette._fields_)
    assert [f for f, _ in L.Palette._fields_] == ["entries", "trns_entries", "rgb", "alpha", "truecolor_bytes", "indexed_bytes", "colors", "reserved"]
    assert L.C.sizeof(L.Palette) == 8 + 768 + 256 + 16 + 8

    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip_indexed.h"
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
    assert declared["pngloss_hip_last_palette"] == ["i32", "ptr", "u64", "ptr"]
    assert prototype_differences(L.INDEXED_PROTOTYPES, declared) == []
    # the library exports both, and hip_lib() has given them their prototypes
    import pngloss_amd as P
    for fn in functions:
        assert getattr(P.hip_lib(), fn).argtypes == L.INDEXED_PROTOTYPES[fn][1]


def _tool():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    return exe


@needs_cli
def test_help_names_the_switch():
    r = subprocess.run([_tool(), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--indexed" in r.stdout


@needs_cli
@pytest.mark.parametrize("other", [["--target-size", "10k"], ["--target-psnr", "40"], ["--target-ssim", "0.9"], ["--max-error", "3"]])
def test_switch_is_refused_with_the_searches(other, tmp_path):
    r = subprocess.run([_tool(), "--indexed"] + other + ["x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 4 and r.stderr.startswith("--indexed cannot be combined with"), r.stderr
    assert not os.listdir(tmp_path)


@needs_cli
def test_switch_does_not_change_the_other_argument_errors(tmp_path):
    for args in (["-s", "300", "x.png"], ["-b", "0", "x.png"], ["--bogus"], ["-f", str(tmp_path / "missing.png")]):
        plain = subprocess.run([_tool()] + args, capture_output=True, text=True, cwd=tmp_path)
        flag = subprocess.run([_tool(), "--indexed"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert flag.returncode == plain.returncode and flag.stderr == plain.stderr, args

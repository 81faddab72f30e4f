"""CPU tests of the Python binding against include/pngloss_hip.h: pngloss_amd/lib.py restates the header's structs (STRUCTS) and prototypes
(PROTOTYPES) by hand, and ctypes takes its word for both.  Here the compiler reads the header and says what the layouts and the declarations
are; the two checks are also run on deliberately broken copies, to show that they can fail.  Then the marshalling helpers every wrapper goes
through.  Only the last test needs the built library (pngloss_hip_zlib_bound is host arithmetic); none needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pngloss_amd import lib as L
from tests import util as U

INCLUDE = os.path.join(U.ROOT, "include")
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "pngloss_hip.h")).read(), flags=re.S)
#: name -> field names in order, of every `typedef struct { ... } name;` of the header
HEADER_STRUCTS = {name: [re.search(r"(\w+)\s*(\[\w*\])?\s*$", part).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
                  for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", HEADER, flags=re.S)}
#: every function the header declares
HEADER_FUNCTIONS = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", HEADER)) - {"defined"})


def _compile_and_run(tmp, name, text, compiler):
    """(stdout, None) of the program `text` compiles to, or (None, the compiler's complaint)"""
    src, exe = os.path.join(tmp, name), os.path.join(tmp, name + ".out")
    with open(src, "w") as fh:
        fh.write(text)
    r = subprocess.run(compiler + ["-I", INCLUDE, "-o", exe, src], capture_output=True, text=True)
    if r.returncode:
        return None, r.stderr
    return subprocess.run([exe], capture_output=True, text=True, check=True).stdout, None


def struct_differences(structs, tmp):
    """what of `structs` (header name -> ctypes.Structure) the header does not bear out: a struct without a mirror, field names that are not the
    header's, and every sizeof, offsetof and field size on which gcc and ctypes disagree.  The C program is written from the _fields_ lists."""
    diffs = [f"{name}: no mirror class" for name in HEADER_STRUCTS if name not in structs]
    diffs += [f"{name}: the header defines no such struct" for name in structs if name not in HEADER_STRUCTS]
    structs = {name: cls for name, cls in structs.items() if name in HEADER_STRUCTS}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pngloss_hip.h"', "int main(void) {"]
    for name, cls in structs.items():
        fields = [f[0] for f in cls._fields_]
        if fields != HEADER_STRUCTS[name]:
            diffs.append(f"{name}: fields {fields}, the header has {HEADER_STRUCTS[name]}")
        lines.append(f'    printf("{name} . %zu 0\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f in fields]
    out, err = _compile_and_run(tmp, "layouts.c", "\n".join(lines + ["    return 0;", "}", ""]), ["gcc", "-std=c11"])
    if err is not None:
        return diffs + ["the layout program does not compile: " + err]
    for line in out.splitlines():
        name, field, size, offset = line.split()
        cls = structs[name]
        mine = (C.sizeof(cls), 0) if field == "." else (getattr(cls, field).size, getattr(cls, field).offset)
        if mine != (int(size), int(offset)):
            diffs.append(f"{name} {field}: (size, offset) {mine} in ctypes, {(int(size), int(offset))} in C")
    return diffs


def type_class(t):
    """the class of a ctypes type as a call passes it: void, ptr, bool, f64, or an integer's signedness and width (i32, u64 ...)"""
    if t is None:
        return "void"
    if issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)):
        return "ptr"
    if t is C.c_bool:
        return "bool"
    if t in (C.c_float, C.c_double):
        return "f%d" % (8 * C.sizeof(t))
    if issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ":
        return ("i" if t._type_.islower() else "u") + str(8 * C.sizeof(t))
    return "other"


@pytest.fixture(scope="module")
def declared(tmp_path_factory):
    """name -> [return class, argument classes ...] of every function of the header, as a C++ compiler sees decltype(&function): nothing is linked"""
    text = """
#include <cstdio>
#include <type_traits>
#include "pngloss_hip.h"
template <class T> void put() {
    if constexpr (std::is_void_v<T>) std::printf(" void");
    else if constexpr (std::is_pointer_v<T>) std::printf(" ptr");
    else if constexpr (std::is_same_v<T, bool>) std::printf(" bool");
    else if constexpr (std::is_floating_point_v<T>) std::printf(" f%zu", sizeof(T) * 8);
    else if constexpr (std::is_integral_v<T>) std::printf(" %c%zu", std::is_signed_v<T> ? 'i' : 'u', sizeof(T) * 8);
    else std::printf(" other");
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void show(const char *name) { std::printf("%s", name); put<R>(); (put<A>(), ...); std::printf("\\n"); }
};
int main() {
""" + "".join(f'    Sig<decltype(&{fn})>::show("{fn}");\n' for fn in HEADER_FUNCTIONS) + "    return 0;\n}\n"
    out, err = _compile_and_run(str(tmp_path_factory.mktemp("abi")), "prototypes.cpp", text, ["g++", "-std=c++17"])
    assert err is None, err
    return {line.split()[0]: line.split()[1:] for line in out.splitlines()}


def prototype_differences(prototypes, declared):
    """what of `prototypes` (name -> (restype, [argtypes])) the header's declarations do not bear out"""
    diffs = [f"{name}: no prototype" for name in declared if name not in prototypes]
    diffs += [f"{name}: the header declares no such function" for name in prototypes if name not in declared]
    for name, (restype, argtypes) in prototypes.items():
        if name not in declared:
            continue
        ret, args = declared[name][0], declared[name][1:]
        if type_class(restype) != ret:
            diffs.append(f"{name}: returns {type_class(restype)}, the header has {ret}")
        if len(argtypes) != len(args):
            diffs.append(f"{name}: {len(argtypes)} arguments, the header has {len(args)}")
        diffs += [f"{name}: argument {k} is {type_class(t)}, the header has {a}" for k, (t, a) in enumerate(zip(argtypes, args)) if type_class(t) != a]
    return diffs


def test_every_struct_of_the_header_has_a_mirror_of_the_same_layout(tmp_path):
    assert len(HEADER_STRUCTS) == 16 and set(HEADER_STRUCTS) == set(L.STRUCTS)
    assert HEADER_STRUCTS["pngloss_hip_png_source"][3:6] == ["color_type", "bit_depth", "interlace"]          # (the parser sees `a, b` declarations)
    assert sum(1 + len(f) for f in HEADER_STRUCTS.values()) == 100
    assert struct_differences(L.STRUCTS, str(tmp_path)) == []


@pytest.mark.parametrize("name,field,moved", [("pngloss_hip_result", "unique_symbols", True), ("pngloss_hip_png_source", "interlace", False),
                                              ("pngloss_hip_zstream", "flags", True)])
def test_the_layout_check_reports_a_dropped_field(tmp_path, name, field, moved):
    """moved: the fields behind the dropped one shift, or the struct shrinks.  `interlace` sits in padding: without it no size and no offset
    changes, and only the comparison of the names tells."""
    good = L.STRUCTS[name]
    broken = type("Broken", (C.Structure,), dict(_fields_=[f for f in good._fields_ if f[0] != field]))
    diffs = struct_differences({**L.STRUCTS, name: broken}, str(tmp_path))
    assert diffs and all(d.startswith(name) for d in diffs), diffs
    assert any("fields" in d and "the header has" in d for d in diffs)
    assert any("(size, offset)" in d for d in diffs) == moved, diffs
    assert any("no mirror class" in d for d in struct_differences({k: v for k, v in L.STRUCTS.items() if k != name}, str(tmp_path)))


def test_every_function_of_the_header_has_its_prototype(declared):
    assert len(HEADER_FUNCTIONS) == 49 and set(declared) == set(HEADER_FUNCTIONS) == set(L.PROTOTYPES)
    assert L.ABI_SYMBOLS == tuple(L.PROTOTYPES)
    assert declared["optimize_with_rows"] == ["i32", "ptr", "u32", "u32", "ptr", "bool", "u8", "i64"]      # (the C++ side tells the classes apart)
    assert declared["pngloss_hip_psnr_db"] == ["f64", "ptr", "u32"] and declared["pngloss_hip_pinned_free"] == ["void", "ptr"]
    assert prototype_differences(L.PROTOTYPES, declared) == []


def test_the_prototype_check_reports_a_missing_and_a_narrowed_argument(declared):
    ret, args = L.PROTOTYPES["pngloss_hip_finish"]
    assert prototype_differences({**L.PROTOTYPES, "pngloss_hip_finish": (ret, args[:-1])}, declared) == ["pngloss_hip_finish: 2 arguments, the header has 3"]
    ret, args = L.PROTOTYPES["pngloss_hip_optimize_batch_host"]
    assert args[4] is C.c_long
    narrowed = args[:4] + [C.c_int] + args[5:]
    assert prototype_differences({**L.PROTOTYPES, "pngloss_hip_optimize_batch_host": (ret, narrowed)}, declared) == [
        "pngloss_hip_optimize_batch_host: argument 4 is i32, the header has i64"]
    # what ctypes does without a prototype: an int comes back where the header returns a pointer, and a missing entry is missing
    assert prototype_differences({**L.PROTOTYPES, "pngloss_hip_pinned_alloc": (C.c_int, [C.c_size_t])}, declared) == [
        "pngloss_hip_pinned_alloc: returns i32, the header has ptr"]
    less = {k: v for k, v in L.PROTOTYPES.items() if k != "pngloss_hip_pinned_alloc"}
    assert prototype_differences(less, declared) == ["pngloss_hip_pinned_alloc: no prototype"]


def test_pointer_spellings_count_as_pointers():
    assert {type_class(t) for t in (C.c_void_p, C.c_char_p, C.POINTER(L.Result), C.POINTER(C.c_void_p))} == {"ptr"}
    assert [type_class(t) for t in (None, C.c_bool, C.c_double, C.c_int, C.c_uint, C.c_long, C.c_size_t, C.c_uint8, C.c_uint32)] == [
        "void", "bool", "f64", "i32", "u32", "i64", "u64", "u8", "u32"]


# ---- the marshalling helpers -------------------------------------------------------------------------------------------------------------------

def _two_arrays():
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), rng.integers(0, 256, (3, 7, 4), dtype=np.uint8)]


@pytest.mark.parametrize("want_filters", [True, False])
@pytest.mark.parametrize("inplace", [False, True])
def test_host_image_table_points_at_the_arrays(want_filters, inplace):
    arrays = _two_arrays()
    before = [a.copy() for a in arrays]
    outs, filts, imgs = L._host_images(arrays, want_filters, inplace)
    assert len(imgs) == 2 and [(a is o) for a, o in zip(arrays, outs)] == [inplace] * 2
    for a, o, f, im, (w, h) in zip(before, outs, filts, imgs, [(1, 1), (7, 3)]):
        assert np.array_equal(o, a) and o.flags["C_CONTIGUOUS"]
        assert (im.rgba, im.width, im.height) == (o.ctypes.data, w, h)
        if want_filters:
            assert f.shape == (h,) and f.dtype == np.uint8 and not f.any() and im.row_filters == f.ctypes.data
        else:
            assert f is None and im.row_filters is None
    with pytest.raises(AssertionError):
        L._host_images([np.zeros((4, 4, 4), np.uint8)[:, ::2]], inplace=True)


def test_tables_of_an_empty_batch_have_one_element():
    assert len(L._array(L.Result, 0)) == 1 and len(L._array(L.Result, 1)) == 1 and len(L._array(C.c_int, 5)) == 5
    outs, filts, imgs = L._host_images([])
    assert (outs, filts, len(imgs)) == ([], [], 1)
    lines, ids, rows = L._scanline_buffers([])
    assert (len(lines), ids, rows, L._scanlines_back(lines, ids, rows)) == (1, [], [], [])
    assert len(L._image_descs([])) == 1 and len(L._image_pairs([])) == 1 and len(L._png_sources([])) == 1
    assert len(L._row_pointers(np.zeros((0, 5, 4), np.uint8))) == 1


def test_device_tables_carry_the_tuples():
    descs = L._image_descs([(0x1000, 0, 7, 3), (0x2000, 0x3000, 1, 1)])
    assert [(d.d_rgba, d.d_row_filters, d.width, d.height) for d in descs] == [(0x1000, None, 7, 3), (0x2000, 0x3000, 1, 1)]
    pairs = L._image_pairs([(0x1000, 0x2000, 7, 3), (0, 0, 0, 0)])
    assert [(p.d_a, p.d_b, p.width, p.height) for p in pairs] == [(0x1000, 0x2000, 7, 3), (None, None, 0, 0)]


@pytest.mark.parametrize("color_type,channels", [(0, 1), (4, 2), (2, 3), (6, 4)])
def test_scanline_slice_follows_the_colour_type(color_type, channels):
    outs = _two_arrays()
    lines, ids, rows = L._scanline_buffers(outs)
    for i, (a, f, r) in enumerate(zip(outs, ids, rows)):
        h, w = a.shape[:2]
        assert f.shape == (h,) and r.shape == (h, w * 4)
        assert (lines[i].filter_types, lines[i].scanlines, lines[i].pitch, lines[i].color_type) == (f.ctypes.data, r.ctypes.data, w * 4, -1)
        r[:] = np.arange(w * 4, dtype=np.uint8)
        lines[i].color_type = color_type                           # (what the C call writes)
    back = L._scanlines_back(lines, ids, rows)
    for (ct, f, r), a, i in zip(back, outs, ids):
        h, w = a.shape[:2]
        assert ct == color_type and f is i and r.shape == (h, w * channels)
        assert np.array_equal(r, np.tile(np.arange(w * channels, dtype=np.uint8), (h, 1)))


def test_png_source_table_carries_the_parsed_file():
    p = dict(scanlines=b"\4abcd", width=1, height=1, ctype=3, depth=8, interlace=1, plte=b"\1\2\3\4\5\6", trns=b"\7", zstream=b"")
    q = dict(p, plte=None, trns=None, interlace=0)
    out = np.zeros((1, 1, 4), np.uint8)
    src = L._png_sources([p, q], [out, out])
    assert (src[0].scanlines, src[0].width, src[0].height, src[0].color_type, src[0].bit_depth, src[0].interlace) == (b"\4abcd", 1, 1, 3, 8, 1)
    assert (src[0].palette, src[0].palette_entries, src[0].trns, src[0].trns_bytes, src[0].rgba) == (b"\1\2\3\4\5\6", 2, b"\7", 1, out.ctypes.data)
    assert (src[1].palette, src[1].palette_entries, src[1].trns, src[1].trns_bytes, src[1].interlace) == (None, 0, None, 0, 0)
    dev = L._png_sources([p], scanlines=[b"\4wxyz"])
    assert dev[0].scanlines == b"\4wxyz" and dev[0].rgba is None


def test_result_dictionaries():
    r = L.Result(65, 3, 200, 5, 9)
    assert L._result_dict(r) == dict(status=65, bpp=3, unique_symbols=200, retried_rows=5, repaired_pixels=9)
    assert L._host_result_dict(r) == dict(status=65, bpp=3, unique_symbols=200)


@pytest.mark.parametrize("stream_only", [False, True])
def test_stream_table_has_the_room_the_library_asks_for(stream_only):
    lib = L.hip_lib()
    shapes = [(1, 1), (7, 3)]
    zs, bufs = L._zstreams(lib, shapes, stream_only)
    assert len(zs) == 2
    for z, b, (w, h) in zip(zs, bufs, shapes):
        assert b.dtype == np.uint8 and b.size == lib.pngloss_hip_zlib_bound(w, h) >= (4 * w + 1) * h
        assert (z.data, z.capacity, z.size, z.color_type, tuple(z.blocks), z.flags) == (b.ctypes.data, b.size, 0, -1, (0, 0, 0), int(stream_only))
    assert len(L._zstreams(lib, [])[0]) == 1
    bufs[1][:4] = (0x78, 0xDA, 1, 2)
    zs[1].size, zs[1].color_type, zs[1].blocks[2] = 4, 2, 1         # (what the C call writes)
    assert L._zstreams_back(zs, bufs)[:2] == [(-1, b"", (0, 0, 0)), (2, b"\x78\xda\x01\x02", (0, 0, 1))]

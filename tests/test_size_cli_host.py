"""CPU tests of the tool's --target-size (no GPU compute): the argument handling where no device is needed, and the file-size helper of
pngloss_amd/cli/png_stream_writer.c against the files that writer puts on disk (tests/c/stream_size.c), for every colour type, with and without
pass-through chunks, with zlib's 8192-byte IDAT slices and with a finished stream in one IDAT chunk."""
import os
import subprocess

import numpy as np
import pytest

from pngloss_amd import lib as L
from tests import util as U

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
PNG_INC = "/opt/conda/include"
PNG_LIB = "/lib/x86_64-linux-gnu/libpng16.so.16"
have_png = os.path.exists(os.path.join(PNG_INC, "png.h")) and os.path.exists(PNG_LIB)
pytestmark = pytest.mark.skipif(not have_png, reason="libpng headers/runtime not found on this box: the command line tool is not built")


def _tool():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    return exe


def test_help_names_the_switch():
    r = subprocess.run([_tool(), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--target-size" in r.stdout


def test_bad_values_and_refused_combinations_are_argument_errors(tmp_path):
    """like a bad strength: the tool's exit code for bad arguments, one line on stderr, no file touched"""
    exe = _tool()
    bad_s = subprocess.run([exe, "-s", "abc", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert bad_s.returncode == L.PNGLOSS_INVALID_ARGUMENT
    bad = [["--target-size", v] for v in ("", "x", "k", "%", "-5", "10kB", "10 k", "5%%", "1.5k", "40 %", "10G", "99999999999999999999", "18014398509481984k", "17592186044416M")]
    bad += [["--target-size", "0"], ["--target-size", "0%"], ["--target-size", "0k"]]
    bad += [["--target-size", "50%", extra, val] for extra, val in (("--target-psnr", "35"), ("--target-ssim", "0.9"), ("--max-error", "8"))]
    bad += [["--target-psnr", "35", "--target-size", "4k"]]
    for args in bad:
        r = subprocess.run([exe] + args + ["x.png"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == L.PNGLOSS_INVALID_ARGUMENT, (args, r.returncode, r.stderr)
        assert r.stderr.strip() and len(r.stderr.splitlines()) == 1, (args, r.stderr)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("value", ["1", "4096", "4k", "4K", "3M", "40%", "100%", "250%"])
def test_good_values_get_past_the_argument_checks(value, tmp_path):
    """a well-formed budget is accepted: the tool goes on to the file, which does not exist (a read error, not an argument error); the switch
    combines with the reporting and path switches"""
    r = subprocess.run([_tool(), "--target-size", value, "-s", "40", "--distortion", "--ssim", "--skip-if-larger", "--gpu-read", "--gpu-deflate", "missing.png"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode not in (0, L.PNGLOSS_INVALID_ARGUMENT) and "cannot open" in r.stderr, (value, r.returncode, r.stderr)


def _samples(d):
    from PIL import Image, PngImagePlugin
    rng = np.random.default_rng(6)
    rgba = rng.integers(0, 256, (23, 31, 4), dtype=np.uint8)
    out = []

    def save(name, im, **kw):
        p = str(d / name)
        im.save(p, **kw)
        out.append(p)

    meta = PngImagePlugin.PngInfo()
    meta.add_text("Comment", "carried through unless --strip")
    gray = np.stack([rgba[..., 1]] * 3 + [np.full((23, 31), 255, np.uint8)], axis=-1)
    graya = np.stack([rgba[..., 1]] * 3 + [rgba[..., 3]], axis=-1)
    rgb = rgba.copy()
    rgb[..., 3] = 255
    for name, a in (("rgba", rgba), ("rgb", rgb), ("gray", gray), ("graya", graya)):              # colour types 6, 2, 0, 4 on the way out
        save(name + ".png", Image.fromarray(a, "RGBA"))
        save(name + "_text_dpi.png", Image.fromarray(a, "RGBA"), pnginfo=meta, dpi=(72, 72))
    save("rgb_gamma.png", Image.fromarray(rgb[..., :3].copy(), "RGB"), gamma=0.5)
    big = rng.integers(0, 256, (200, 300, 4), dtype=np.uint8)                                     # 240 KB of noise: many 8192-byte IDAT slices
    save("big_text.png", Image.fromarray(big, "RGBA"), pnginfo=meta)
    save("one_pixel.png", Image.fromarray(rgba[:1, :1].copy(), "RGBA"))
    return out


def test_predicted_file_size_equals_the_file_on_disk(tmp_path):
    exe = str(tmp_path / "stream_size")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-I" + PNG_INC, "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "stream_size.c"),
                    os.path.join(CLI, "png_bridge.c"), os.path.join(CLI, "png_stream_writer.c"), PNG_LIB, "-lz", "-lm"], check=True, capture_output=True)
    sliced = with_chunks = 0
    for src in _samples(tmp_path):
        sizes = {}
        for strip in (0, 1):
            a, b = src[:-4] + ".zlib.png", src[:-4] + ".stream.png"
            r = subprocess.run([exe, src, a, b, str(strip)], capture_output=True, text=True)
            assert r.returncode == 0, (src, strip, r.stderr)
            p1, n1, p2, n2, zsize, at, below, none, one = map(int, r.stdout.split())
            assert p1 == n1 == os.path.getsize(a), (src, strip)             # zlib's stream in 8192-byte slices
            assert p2 == n2 == os.path.getsize(b), (src, strip)             # a finished stream in one chunk
            assert (at, below, none, one) == (zsize, zsize - 1, 0, 1), (src, strip)
            sliced += os.path.getsize(a) > 3 * 8192
            sizes[strip] = n2
        with_chunks += sizes[0] > sizes[1]
    assert sliced >= 1 and with_chunks >= 4                                  # several IDAT slices, and pass-through chunks that --strip drops

"""CPU test of the lines the command line tool prints about one written file (pngloss_amd/cli/cli_report.c; no GPU): hand-made records through
tests/c/cli_report_host.c must give exactly what the Python mirrors of the GPU tests say (tests/util_distort.cli_line, tests/util_ssim.cli_line,
tests/util_visible.cli_lines); the lines without a mirror must equal the strings below, which are the tool's format strings as they were before
the lines moved out of its main file."""
import os
import subprocess

import pytest

from tests import util as U
from tests import util_distort as D
from tests import util_ssim as S
from tests import util_visible as V

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")
NONE, QUALITY, SIZE = 0, 1, 2


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """lines of the driver's input -> the tool's lines about them"""
    exe = str(tmp_path_factory.mktemp("cli_report") / "cli_report_host")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", exe, os.path.join(U.ROOT, "tests", "c", "cli_report_host.c"),
                    os.path.join(CLI, "cli_report.c"), "-L" + CSRC, "-lpngloss_hip", "-Wl,-rpath," + CSRC, "-lm"], check=True, capture_output=True)

    def run(records):
        r = subprocess.run([exe], input="".join(line + "\n" for line in records), capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        out = r.stdout.split("--\n")
        assert out[-1] == "" and len(out) == len(records) + 1
        return out[:-1]

    return run


def _distortion(bpp, visible, rec):
    return "distortion %d %d %d %d %s %s" % (bpp, visible, rec["pixels"], rec["changed_pixels"], " ".join(map(str, rec["sq_err"])), " ".join(map(str, rec["max_abs"])))


def _ssim(have, search, bpp, visible, rec):
    return "ssim %d %d %d %d %d %s %s" % (have, search, bpp, visible, rec["windows"], " ".join(map(str, rec["sum_q16"])), " ".join(map(str, rec["min_q16"])))


#: distortion records: changed (every channel with its own error, so that a wrong channel mask shows), unchanged, one of 2^33 pixels, no pixels
CHANGED = dict(pixels=1200, changed_pixels=37, sq_err=[900, 4, 160000, 25], max_abs=[9, 2, 200, 5])
UNCHANGED = dict(pixels=1200, changed_pixels=0, sq_err=[0, 0, 0, 0], max_abs=[0, 0, 0, 0])
HUGE = dict(pixels=2 ** 33, changed_pixels=2 ** 32 + 5, sq_err=[2 ** 40, 3, 2 ** 41, 7], max_abs=[255, 1, 254, 2])
#: SSIM records: every channel with its own sum and worst window; a negative worst window; zero windows
WINDOWS = dict(windows=31 * 16, sum_q16=[31 * 16 * 65536, 31 * 16 * 60000, 31 * 16 * 40000, 31 * 16 * 65000], min_q16=[65536, 51234, 1200, 64000], reserved=0)
NEGATIVE = dict(windows=4, sum_q16=[4 * 30000, -4 * 2000, 4 * 65536, 4 * 100], min_q16=[10, -40000, 65536, -3], reserved=0)
NO_WINDOWS = dict(windows=0, sum_q16=[0] * 4, min_q16=[65536] * 4, reserved=0)


def test_channel_mask_is_the_one_of_the_mirrors(ask):
    assert ask(["mask %d" % bpp for bpp in (1, 2, 3, 4)]) == ["%x\n" % D.PSNR_MASK_OF_BPP[bpp] for bpp in (1, 2, 3, 4)]


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_distortion_and_ssim_lines_equal_the_mirrors(ask, bpp):
    for rec in (CHANGED, UNCHANGED, HUGE):
        assert ask([_distortion(bpp, 0, rec)]) == [D.cli_line(rec, bpp) + "\n"]
    for rec in (WINDOWS, NEGATIVE, NO_WINDOWS):
        for search in (NONE, QUALITY):         # a record is a record, whichever call it came from
            assert ask([_ssim(1, search, bpp, 0, rec)]) == [S.cli_line(rec, bpp) + "\n"]
    for rec in (CHANGED, UNCHANGED, HUGE):
        for srec in (WINDOWS, NEGATIVE, NO_WINDOWS):
            assert ask([_distortion(bpp, 1, rec), _ssim(1, NONE, bpp, 1, srec)]) == [line + "\n" for line in V.cli_lines(rec, srec, bpp)]


def test_a_negative_worst_window_and_a_masked_channel_show_in_the_text(ask):
    """the mirrors agree with the tool above; this pins that the cases are what they are meant to be"""
    assert ask([_ssim(1, NONE, 2, 0, NEGATIVE)]) == ["  ssim: mean -0.0145, worst window -0.6104, 4 windows\n"]
    assert ask([_distortion(1, 0, CHANGED)]) == ["  distortion: PSNR %.2f dB, 37 of 1200 pixels changed, largest channel error 2\n" % D.py_psnr_db(CHANGED, 0x2)]
    assert ask([_distortion(3, 0, CHANGED)])[0].endswith("largest channel error 200\n")


def test_lines_without_a_mirror(ask):
    """the strings are the format strings of say_ssim and encode_job as they stood in pngloss_main.c"""
    assert ask([_ssim(0, SIZE, 4, 0, NO_WINDOWS), _ssim(0, SIZE, 4, 1, WINDOWS)]) == ["  ssim: not measured (the size search keeps no SSIM record)\n"] * 2
    assert ask([_ssim(0, QUALITY, 4, 0, NO_WINDOWS), _ssim(0, QUALITY, 1, 1, WINDOWS)]) == ["  ssim: not measured (a strength search measures it only with --target-ssim)\n"] * 2
    assert ask([_ssim(0, NONE, 4, 0, WINDOWS)]) == [""]                  # the library had no record and there was no search: no line
    assert ask(["strength 19 1", "strength 0 9"]) == ["  strength %u chosen in %u probes\n".replace("%u", "%d") % t for t in ((19, 1), (0, 9))]
    fmt = "  indexed: %d colours, %d bytes of image data and %d of palette against %d bytes as truecolour\n"
    # PLTE costs 12 bytes of framing and 3 per entry; tRNS, where there is one, 12 and 1 per entry (tests/util_index.overhead)
    assert ask(["indexed 194 12231 194 0 29980", "indexed 5 100 5 2 90000000000", "indexed 256 7 256 256 9"]) == [
        fmt % (194, 12231, 12 + 3 * 194, 29980), fmt % (5, 100, 12 + 15 + 12 + 2, 90000000000), fmt % (256, 7, 12 + 768 + 12 + 256, 9)]
    assert ask(["budget dir/a.png 5120 6001 40", "budget b.png 1 99 0"]) == [
        "  warning: dir/a.png: budget of 5120 bytes not reached, wrote 6001 bytes at strength 40\n",
        "  warning: b.png: budget of 1 bytes not reached, wrote 99 bytes at strength 0\n"]

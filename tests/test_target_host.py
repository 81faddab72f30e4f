"""CPU tests of the strength search (no GPU compute): the rule of pngloss_amd/csrc/pl_target.h and the thread loop of its copy kernel
(pl_move_core.h), run on the CPU under the sanitizers (tests/c/target_host.cpp) against a restatement of the rule in Python
(tests/util_target.py); the argument checks, the exported symbols and the command line switches where no device is needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_target as T

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists("/opt/conda/include/png.h") or os.path.exists("/usr/include/png.h")
needs_cli = pytest.mark.skipif(not have_png, reason="libpng headers not found on this box: the command line tool is not built")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("target_host")
    return T.build_target_host(d), d


def _table(bits):
    return "".join("1" if b else "0" for b in bits)


def test_search_rule_for_every_bound_monotone_and_random_tables(harness):
    """every M in 0..255: the monotone tables with every threshold (strengths below t pass), and random non-monotone ones.  Per case the probe
    sequence, the chosen strength, the probe count and the bound 1 + ceil(log2 M)."""
    exe, d = harness
    rng = np.random.default_rng(17)
    cases = []
    for m in range(256):
        for t in range(m + 2):                                   # strengths < t are accepted: t = 0 nothing, t = m + 1 everything
            cases.append((m, [s < t for s in range(m + 1)]))
    for _ in range(400):
        m = int(rng.integers(0, 256))
        cases.append((m, list(rng.random(m + 1) < rng.random())))
    got = T.run_target_host(exe, d, ["S %d %s" % (m, _table(tb)) for m, tb in cases])
    reached_bound = set()
    for (m, tb), line in zip(cases, got):
        v = [int(x) for x in line.split()]
        chosen, seq = T.py_search(m, lambda s: tb[s])
        assert v[0] == chosen and v[3:] == seq and v[1] == len(seq), (m, _table(tb), line)
        assert v[2] == T.py_probe_bound(m) and len(seq) <= v[2], (m, line)
        assert all(0 <= s <= m for s in seq) and len(set(seq)) == len(seq)       # never above M, no strength probed twice
        assert chosen == 0 or tb[chosen]                                       # a chosen strength above 0 was probed and accepted
        if len(seq) == v[2]:
            reached_bound.add(m)
    assert reached_bound == set(range(256))                      # the bound is attained for every M
    assert [T.py_probe_bound(m) for m in (0, 1, 2, 3, 4, 5, 19, 40, 128, 129, 255)] == [1, 1, 2, 3, 3, 4, 6, 7, 8, 9, 9]


def test_a_probe_with_a_status_ends_the_search_at_its_strength(harness):
    exe, d = harness
    tb = _table([s < 12 for s in range(20)])
    seq = T.py_search(19, lambda s: s < 12)[1]
    assert seq == [19, 9, 14, 11, 12]
    got = T.run_target_host(exe, d, ["F 19 %s %d" % (tb, k) for k in range(1, len(seq) + 1)])
    for k, line in enumerate(got, start=1):
        assert [int(x) for x in line.split()] == [seq[k - 1], k, 1] + seq[:k], line


def _accept_cmd(psnr, max_abs, status, bpp, pixels, sq, mx, changed=1):
    return "A %s %d 19 %d %d %d %d %s %s" % (T.double_bits(psnr), max_abs, status, bpp, pixels, changed, " ".join(map(str, sq)), " ".join(map(str, mx)))


def test_acceptance_on_hand_made_records(harness):
    exe, d = harness
    # 100 pixels, error 5 in every sample of one channel: PSNR over that channel alone 34.15 dB, over a mask of k channels + 10 log10(k)
    cases = []

    def case(want, *a, **k):
        cases.append((want, _accept_cmd(*a, **k)))

    only = lambda c, v: [v if i == c else 0 for i in range(4)]
    # each mask: bpp 1 looks at G alone, 2 at G and A, 3 at R, G, B, 4 at all
    for bpp, mask in ((1, 0x2), (2, 0xA), (3, 0x7), (4, 0xF)):
        for c in range(4):
            inside = bool(mask >> c & 1)
            k = bin(mask).count("1")
            psnr = 10 * math.log10(65025.0 * k / 25.0)
            case(True, 30.0, 0, 0, bpp, 100, only(c, 2500), only(c, 5))
            case(not inside, psnr + 0.01, 0, 0, bpp, 100, only(c, 2500), only(c, 5))     # error only outside the mask: PSNR is infinite
            case(True, psnr - 0.01, 0, 0, bpp, 100, only(c, 2500), only(c, 5))
            case(not inside, math.inf, 0, 0, bpp, 100, only(c, 2500), only(c, 5))
            # the max_abs_error edge: equal passes, one above fails -- inside the mask only
            case(True, 0.0, 5, 0, bpp, 100, only(c, 2500), only(c, 5))
            case(not inside, 0.0, 4, 0, bpp, 100, only(c, 2500), only(c, 5))
            case(not inside, 30.0, 4, 0, bpp, 100, only(c, 2500), only(c, 5))            # both conditions: the second one decides
    case(True, math.inf, 0, 0, 4, 100, [0] * 4, [0] * 4, changed=0)                      # + inf: a lossless result passes
    case(False, math.inf, 0, 0, 4, 100, [0, 0, 0, 1], [0, 0, 0, 1])
    case(True, 0.0, 0, 0, 4, 100, [2500] * 4, [255] * 4)                                 # no condition at all
    case(True, math.inf, 1, 0, 4, 0, [0] * 4, [0] * 4, changed=0)                        # an image without pixels
    case(True, 60.0, 1, 0, 0, 0, [0] * 4, [0] * 4, changed=0)
    case(False, 0.0, 0, 65, 4, 100, [0] * 4, [0] * 4, changed=0)                         # status not 0
    case(False, 0.0, 0, 65, 4, 0, [0] * 4, [0] * 4, changed=0)
    got = T.run_target_host(exe, d, [c for _, c in cases])
    for (want, cmd), line in zip(cases, got):
        assert line == ("1" if want else "0"), cmd
    # and the Python restatement the other tests rely on agrees on the same records
    for want, cmd in cases:
        f = cmd.split()
        rec = dict(pixels=int(f[6]), changed_pixels=int(f[7]), sq_err=[int(x) for x in f[8:12]], max_abs=[int(x) for x in f[12:16]])
        import struct
        psnr = struct.unpack("<d", struct.pack("<Q", int(f[1], 16)))[0]
        assert T.py_accept(psnr, int(f[2]), rec, int(f[4]), int(f[5])) == want, cmd


def test_groups_of_a_round_and_the_arena_layout(harness):
    exe, d = harness
    shapes = [(3, 2), (0, 0), (64, 8), (257, 5), (1, 1), (0, 7)]
    flat = " ".join("%d %d" % s for s in shapes)
    got = T.run_target_host(exe, d, ["G 19 9 -1 19 0 9 255", "G -1 -1", "L 0 " + flat, "L 1 " + flat])
    assert got[0] == "0:4 9:1,5 19:0,3 255:6" and got[1] == ""
    for host, line in ((0, got[2]), (1, got[3])):
        v = [int(x) for x in line.split()]
        total, moves, jobs, records = v[:4]
        n = len(shapes)
        ranges = [(moves, 24 * 3 * n), (jobs, 32 * n), (records, 64 * n)]
        for i, (w, h) in enumerate(shapes):
            orig, best, bestf, img, filt = v[4 + 5 * i: 9 + 5 * i]
            rows = h if w else 0
            ranges += [(orig, w * h * 4), (best, w * h * 4), (bestf, rows)]
            if host:
                ranges += [(img, w * h * 4), (filt, rows)]
        assert all(a % 256 == 0 for a, _ in ranges)
        live = sorted((a, a + b) for a, b in ranges if b)
        assert all(x[1] <= y[0] for x, y in zip(live, live[1:])) and live[-1][1] <= total      # nothing overlaps, everything inside


def test_move_thread_loop_under_asan_and_ubsan(harness):
    """the copy kernel's thread loop: sizes around the 16-byte and word steps, every pair of alignments that takes another path, few and many threads"""
    exe, d = harness
    cmds = []
    for nbytes in (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 64, 1000, 4097, 130 * 6 * 4, 130 * 6):
        for so, do in ((0, 0), (4, 0), (0, 4), (4, 12), (1, 0), (0, 3), (2, 2), (8, 8)):
            for nt in (1, 7, 256, 2048):
                cmds.append("M %d %d %d %d" % (nbytes, so, do, nt))
    assert set(T.run_target_host(exe, d, cmds)) == {"1"}


def test_bad_targets_are_refused_without_a_device(harness):
    exe, d = harness
    bad = [(math.nan, 0, 19), (-1.0, 0, 19), (-math.inf, 0, 19), (35.0, 256, 19), (35.0, 0, 256)]
    good = [(0.0, 0, 0), (35.0, 0, 19), (math.inf, 255, 255), (0.0, 8, 40)]
    got = T.run_target_host(exe, d, ["C %s %d %d" % (T.double_bits(p), e, m) for p, e, m in bad + good])
    assert got == [str(L.PNGLOSS_INVALID_ARGUMENT)] * len(bad) + ["0"] * len(good)
    lib = P.hip_lib()
    for p, e, m in bad:
        t = P.Target(p, e, m)
        assert lib.pngloss_hip_optimize_batch_target(None, None, 0, C.byref(t), 2, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_multi_optimize_batch_host_target(None, None, 0, C.byref(t), 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_optimize_batch_target(None, None, 0, None, 2, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT


def test_both_entry_points_are_exported_and_declared():
    header = open(os.path.join(U.ROOT, "include", "pngloss_hip.h")).read()
    lib = C.CDLL(os.path.join(U.ROOT, "pngloss_amd", "csrc", "libpngloss_hip.so"))
    for name in ("pngloss_hip_optimize_batch_target", "pngloss_hip_multi_optimize_batch_host_target"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in L.ABI_SYMBOLS, name
    for name in ("pngloss_hip_target", "pngloss_hip_target_report"):
        assert re.search(r"\}\s*%s\s*;" % name, header), name
    assert C.sizeof(P.Target) == 16 and C.sizeof(P.TargetReport) == 16 + C.sizeof(P.Distortion)


def _tool():
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    return exe


@needs_cli
def test_help_names_both_switches():
    r = subprocess.run([_tool(), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--target-psnr" in r.stdout and "--max-error" in r.stdout


@needs_cli
def test_bad_switch_values_are_refused_like_a_bad_strength(tmp_path):
    exe = _tool()
    bad_s = subprocess.run([exe, "-s", "abc", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    range_s = subprocess.run([exe, "-s", "300", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert bad_s.returncode == range_s.returncode == L.PNGLOSS_INVALID_ARGUMENT
    for args, like in ((["--target-psnr", "x"], bad_s), (["--target-psnr", ""], bad_s), (["--target-psnr", "35dB"], bad_s), (["--max-error", "x"], bad_s),
                       (["--target-psnr", "-1"], range_s), (["--target-psnr", "nan"], range_s), (["--max-error", "256"], range_s), (["--max-error", "0"], range_s)):
        r = subprocess.run([exe] + args + ["x.png"], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == like.returncode, (args, r.stderr)
        assert r.stderr.strip() and len(r.stderr.splitlines()) == len(like.stderr.splitlines()) == 1, (args, r.stderr)      # one line of message, no file touched
    assert not os.listdir(tmp_path)

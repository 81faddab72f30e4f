"""Helpers of the colour-count search tests (tests/test_quant_target_host.py, tests/test_gpu_quant_target.py): the procedure of
include/pngloss_hip_quant_target.h restated in Python over the restatements of the quantiser (tests/util_quant.py, tests/util_dither.py), and the
builders of the two CPU harnesses.  Nothing here calls the code under test for an expected value."""
import functools
import math
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_distort as D
from tests import util_dither as F
from tests import util_quant as Q
from tests.util_quant import from_words, words  # noqa: F401

MAX_PROBES = 12


# ---- the rule ----

def probe_bound(m):
    """1 + ceil(log2(M - 1))"""
    return 1 + (0 if m <= 2 else math.ceil(math.log2(m - 1)))


def search(accepted, m):
    """the procedure over accepted(N) -> bool: dict(colors, reached, probes, probed, accepted_mask)"""
    probed, mask = [], 0

    def probe(n):
        nonlocal mask
        ok = bool(accepted(n))
        mask |= int(ok) << len(probed)
        probed.append(n)
        return ok

    if not probe(m):
        return dict(colors=m, reached=0, probes=1, probed=probed, accepted_mask=mask)
    lo, hi = 1, m
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            hi = mid
        else:
            lo = mid
    return dict(colors=hi, reached=1, probes=len(probed), probed=probed, accepted_mask=mask)


def accepts(rec, min_psnr_db=0.0, max_abs_error=0):
    """the acceptance rule over a record dict (D.np_distortion's)"""
    if rec["pixels"] == 0:
        return True
    if min_psnr_db != 0.0 and not D.py_psnr_db(rec, 0xF) >= min_psnr_db:
        return False
    if max_abs_error and max(rec["max_abs"]) > max_abs_error:
        return False
    return True


class Probes:
    """the probes of one image at one `rounds` and `dither`, each restated once and kept: at(N) is Q.restate's (or F.restate's) dict"""

    def __init__(self, img, rounds=8, dither=0):
        self.img, self.rounds, self.dither = np.ascontiguousarray(img, dtype=np.uint8), rounds, dither
        self.at = functools.lru_cache(maxsize=None)(self._at)

    def _at(self, n):
        return (F.restate if self.dither else Q.restate)(self.img, n, self.rounds)

    def psnr(self, n):
        return D.py_psnr_db(self.at(n)["distortion"], 0xF)

    def search(self, m, min_psnr_db=0.0, max_abs_error=0):
        """the restated procedure: search()'s dict, and under "quant" the restated report at the chosen N"""
        out = search(lambda n: accepts(self.at(n)["distortion"], min_psnr_db, max_abs_error), m)
        out["quant"] = self.at(out["colors"])
        return out

    def margin(self, got, min_psnr_db):
        """how far the PSNR target is from the nearest probed PSNR, in dB: C's and Python's log10 must not disagree on a probe"""
        finite = [abs(self.psnr(n) - min_psnr_db) for n in got["probed"] if math.isfinite(self.psnr(n)) and math.isfinite(min_psnr_db)]
        return min(finite) if finite else math.inf


def same_report(name, got, want):
    """a report dict of the library (QuantTargetReport.as_dict) against the restated search"""
    assert (got["colors"], got["reached"], got["probes"], got["probed"], got["accepted_mask"]) == \
           (want["colors"], want["reached"], want["probes"], want["probed"], want["accepted_mask"]), (name, got, {k: v for k, v in want.items() if k != "quant"})
    q, w = got["quant"], want["quant"]
    assert q["status"] == 0 and (q["colors_in"], q["entries"], q["exact"]) == (w["colors_in"], w["entries"], w["exact"]), name
    assert q["palette"] == w["palette"] and q["distortion"] == w["distortion"], name


# ---- tests/c/colors_host.cpp: pl_colors.h on the CPU ----

def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", name + ".cpp")] + list(extra), check=True, capture_output=True)
    return exe


def build_colors_host(tmp_path):
    return _build(tmp_path, "colors_host")


def build_measure_host(tmp_path):
    return _build(tmp_path, "quant_measure_host", ["-lpthread"])


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def run_colors_host(exe, tmp_path, commands):
    """one answer line per command line"""
    path = str(tmp_path / "colors_commands.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(commands) + "\n")
    lines = _run(exe, [path]).splitlines()
    assert len(lines) == len(commands)
    return lines


def double_bits(v):
    return np.array([v], np.float64).view(np.uint64)[0].item().to_bytes(8, "big").hex()


# ---- tests/c/quant_measure_host.cpp: the lane loop of pl_quant_measure on the CPU ----

def measure_constants(exe):
    return [int(v) for v in _run(exe, ["constants"]).split()]


def run_measure_host(exe, tmp_path, cases):
    """cases: (image (H, W, 4) uint8, palette [words], blocks, lanes, team, offset_words).  Returns per case the record dict without `pixels` (the
    host's to write); fails on any sanitizer report."""
    path, out_path = str(tmp_path / "measure_cases.bin"), str(tmp_path / "measure_out.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for img, pal, blocks, lanes, team, offset in cases:
            fh.write(np.array([img.shape[1], img.shape[0], len(pal), blocks, lanes, team, offset], np.uint32).tobytes())
            fh.write(np.array(pal, np.uint32).tobytes())
            fh.write(words(img).tobytes())
    _run(exe, ["run", path, out_path])
    raw = np.fromfile(out_path, np.uint64).reshape(len(cases), 9)
    return [dict(changed_pixels=int(r[0]), sq_err=[int(v) for v in r[1:5]], max_abs=[int(v) for v in r[5:9]]) for r in raw]

"""Helpers of the size tests (tests/test_size_host.py, tests/test_size_oracle.py, tests/test_gpu_size.py): the rule of
pngloss_hip_optimize_batch_size restated in Python, the CPU chain that gives a probe's stream size, the pinned table and the builders of the CPU
harnesses.  Nothing here calls the code under test."""
import functools
import json
import math
import os
import subprocess

import numpy as np

from tests import util as U
from tests import util_target as T

BLEED = T.BLEED
TABLE = os.path.join(U.GOLDEN, "size_target_table.json")


def py_probe_bound(m):
    """1 + ceil(log2(M + 1))"""
    return 1 + math.ceil(math.log2(m + 1))


def py_search(m, accepted):
    """the rule: accepted(strength) -> bool is asked once per probe.  Returns (chosen, reached, probe sequence)."""
    seq = [m]
    if not accepted(m):
        return m, 0, seq
    lo, hi = -1, m
    while hi - lo > 1:
        mid = (lo + hi) // 2
        seq.append(mid)
        if accepted(mid):
            hi = mid
        else:
            lo = mid
    return hi, 1, seq


def scanline_bytes(out, filt, filters=True):
    """(colour type, the bytes a PNG encoder deflates) for an optimised image and its row filter flags"""
    ctype, ids, rows = U.png_scanlines_reference(out, filt if filters else None)
    return ctype, b"".join(bytes([int(t)]) + r.tobytes() for t, r in zip(ids, rows))


@functools.lru_cache(maxsize=None)
def oracle_size(w, h, mode, strength, frame=0):
    """(stream bytes, colour type) of synth_rgba(w, h, mode, frame) at `strength`: run_port -> png_scanlines_reference -> deflate_host -> length;
    cached, so every test shares one computation"""
    _, out, filt, _, _ = T.oracle_probe(w, h, mode, strength, frame)
    if not out.size:
        return 0, 6
    ctype, raw = scanline_bytes(out, filt)
    z, _ = U.deflate_host(raw)
    return len(z), ctype


def oracle_search(shape, m, budget):
    """the rule on the CPU chain: (chosen, reached, probe sequence, bytes of the kept result)"""
    w, h, mode = shape
    if not w * h:
        return 0, 1, [], 0
    chosen, reached, seq = py_search(m, lambda s: oracle_size(w, h, mode, s)[0] <= budget)
    return chosen, reached, seq, oracle_size(w, h, mode, chosen)[0]


def load_table():
    with open(TABLE) as fh:
        return json.load(fh)


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(U.ROOT, "tests", "c", name + ".cpp")] + list(extra), check=True, capture_output=True)
    return exe


def build_size_host(tmp_path):
    """tests/c/size_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "size_host")


def build_deal_host(tmp_path):
    """tests/c/deal_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "deal_host")


def build_search_host(tmp_path):
    """tests/c/search_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "search_host")


def build_pace_host(tmp_path):
    """tests/c/pace_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "pace_host")


def build_deflate_measure_host(tmp_path):
    """tests/c/deflate_measure_host.cpp with -fsanitize=address,undefined; returns the executable"""
    return _build(tmp_path, "deflate_measure_host", ["-lpthread"])


def run_host(exe, tmp_path, commands, timeout=600):
    """one answer line per command line; fails on any sanitizer report"""
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(commands) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(commands)
    return lines

"""The step counts of the segment enumeration are compile-time values (pl_seg_core.h: seg_enum_body_k<NT, K1>, seg_run_fast<F, TRX, N>) and a step forms
its shared-memory addresses from operands made once per run (SegStepMem).  The CPU harness (tests/c/seg_host.cpp) runs the same bodies; what these
tests add to tests/test_seg_host.py are the corners that change can break: a second build of the harness with -DSEG_K1_ONE_CHUNK=2 -- a count other
than 4 before the dedupe, a leg of SEG_PL - 2 steps behind it, and the body's one branch between two different counts --, widths around one segment
(32 pixels) and around a row of one, two, three and nine segments, every byte-per-pixel class, fully transparent pixels (the TRX variants of every
run), NULL row_filters, a state set of one chunk (s=19 b=2) and one of three (s=20 b=1: 739 states, the SEG_K1 path).  Bar: the oracle's bytes and filter IDs."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

WIDTHS = (1, 31, 32, 33, 65, 257)
HEIGHTS = (4, 5, 6)
MODES = (0, 2, 3, 4, 5)          # 4, 3, 2, 1 bytes per pixel; 5: four bytes with fully transparent pixels on an 8x8 checkerboard


@functools.lru_cache(maxsize=None)
def _want(w, h, mode, s, b, filters):
    out, f = U.run_port(P.synth_rgba(w, h, mode, 0), s, b, filters=filters)
    out.setflags(write=False)
    return out, f


@pytest.fixture(scope="module")
def harness_k1_2(tmp_path_factory):
    """the harness of tests/util.py, built from the same sources with two steps before the dedupe where the state set fits one chunk"""
    so = tmp_path_factory.mktemp("seg_host_k1_2") / "libseg_host_k1_2.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-DSEG_K1_ONE_CHUNK=2", "-o", str(so), os.path.join(U.ROOT, "tests", "c", "seg_host.cpp")], check=True)
    lib = C.CDLL(str(so))
    lib.seg_host_optimize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint, C.c_long, C.c_void_p]
    lib.seg_host_optimize.restype = C.c_int
    return lib


def _run(lib, img, s, b, filters):
    out = np.ascontiguousarray(img).copy()
    h, w, _ = out.shape
    f = np.zeros(h, np.uint8)
    st = np.zeros(8, np.uint32)
    rc = lib.seg_host_optimize(out.ctypes.data, w, h, f.ctypes.data if filters else None, s, b, st.ctypes.data)
    return rc, out, f, st


@pytest.mark.parametrize("filters", [True, False], ids=["ids", "null"])
@pytest.mark.parametrize("s,b,states", [(19, 2, 253), (20, 1, 739)])
@pytest.mark.parametrize("build", ["k1_4", "k1_2"])
def test_enumeration_with_compile_time_step_counts_matches_oracle(build, s, b, states, filters, harness_k1_2):
    lib = U.seg_host_lib() if build == "k1_4" else harness_k1_2
    for w in WIDTHS:
        for h in HEIGHTS:
            for mode in MODES:
                rc, out, f, st = _run(lib, P.synth_rgba(w, h, mode, 0), s, b, filters)
                want, wf = _want(w, h, mode, s, b, filters)
                assert rc == 0 and int(st[6]) == states, (w, h, mode, st)
                assert np.array_equal(out, want), (build, w, h, mode)
                if filters:
                    assert np.array_equal(f, wf), (build, w, h, mode)

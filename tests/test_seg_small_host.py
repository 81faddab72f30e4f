"""The enumeration body of none / up (pngloss_amd/csrc/pl_seg_core.h: seg_enum_small_body) on the CPU: its TABLE PATH -- one step per pixel record and value of cn, then a
walk of lookups -- against its step loop, which is the parent's body.  tests/c/seg_small_host.cpp puts a hook in the body's place inside the CPU harness's launches
(tests/c/seg_host.cpp): every call runs both on the same job and compares every record they leave (maps, dcnt, rck, rout, rst); the image goes on with the shipped body.
Whole images are checked against the restatement's bytes and filter IDs, and the attempts against a run with the loop alone.

(strength, bleed) pairs and what the body does with them: SEG_SMALL_NCN values of cn fit a workgroup -- 16 at 512 threads, 7 at 1024 -- so
   (19, 2)  17 states, cmax 4: tables at 512 threads, the loop at 1024          (7, 1)   7 states, cmax 3: tables at both, the largest set that takes them at 1024
   (15, 1)  21 states, cmax 6: the largest small set there is, tables at 512     (8, 1)  15 states, cmax 4: just beyond at 1024 -- the loop --, tables at 512
   (20, 1)  no small set at all: none / up go through seg_enum_body, the hook is never called."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

SRC = os.path.join(U.ROOT, "tests", "c", "seg_small_host.cpp")
#        s, b: ns_small, tables at 512, tables at 1024
PAIRS = {(19, 2): (17, 1, 0), (7, 1): (7, 1, 1), (15, 1): (21, 1, 0), (8, 1): (15, 1, 0), (20, 1): (0, 0, 0)}
WIDTHS = (1, 31, 32, 33, 127, 128, 129, 257)
MODES = (0, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("seg_small") / "libseg_small_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.seg_small_host_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint, C.c_long, C.c_int, C.c_void_p, C.c_void_p]
    lib.seg_small_host_run.restype = C.c_int
    lib.seg_small_host_describe.argtypes = [C.c_uint, C.c_long, C.c_void_p]
    lib.seg_small_host_describe.restype = C.c_int
    return lib


def run(lib, img, s, b, mode, filters=True):
    """-> rc, out, filter ids, stats (attempts first), counts (calls, differing records, lanes walked, lanes of the table path in the loop, of these back in the set,
    lanes of a body without tables, ns_small, tables fit)"""
    out = np.ascontiguousarray(img).copy()
    h, w, _ = out.shape
    f, st, cnt = np.zeros(h, np.uint8), np.zeros(8, np.uint32), np.zeros(8, np.uint64)
    rc = lib.seg_small_host_run(out.ctypes.data, w, h, f.ctypes.data if filters else None, s, b, mode, st.ctypes.data, cnt.ctypes.data)
    return rc, out, (f if filters else None), st, [int(v) for v in cnt]


def test_which_sets_take_the_tables(lib):
    for (s, b), want in PAIRS.items():
        d = np.zeros(4, np.int32)
        assert lib.seg_small_host_describe(s, b, d.ctypes.data) == 0
        assert (int(d[0]), int(d[2]), int(d[3])) == want and int(d[1]) == (want[0] > 0), (s, b, list(d))
    # no set with small_ok is larger than (15, 1)'s: at 512 threads every one of them takes the tables
    for s in range(0, 128):
        for b in (1, 2, 3, 4, 8, 16, 32767):
            d = np.zeros(4, np.int32)
            if lib.seg_small_host_describe(s, b, d.ctypes.data) == 0 and d[1]:
                assert d[0] <= 21 and d[2] == 1, (s, b, list(d))


def test_table_path_leaves_the_loops_records_under_asan_and_ubsan(tmp_path):
    """the harness as a program of its own under -fsanitize=address,undefined, every launch with an LDS buffer of exactly its bytes: widths 1 .. 257 x heights 4 .. 6 x modes
    0, 2, 3, 4, 5 x both workgroup sizes, with and without row filters: all 80 cases at (19, 2), every fifth at the other pairs"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    objs = []
    for src in (os.path.join(U.ROOT, "pngloss_amd", "csrc", "pngloss_synth.c"), os.path.join(U.ROOT, "oracle", "pngloss_port.c")):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        subprocess.run(["gcc", "-std=gnu11", "-Wno-unknown-pragmas", "-Wno-unused-function"] + san + ["-c", "-o", objs[-1], src], check=True, capture_output=True)
    exe = str(tmp_path / "seg_small")
    subprocess.run(["g++", "-std=c++17", "-w", "-DSEG_SMALL_MAIN"] + san + ["-o", exe, SRC] + objs, check=True, capture_output=True)
    args = []
    for (s, b) in PAIRS:
        args += [str(s), str(b), "1" if (s, b) == (19, 2) else "5"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEG_HOST_")}
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900, env=dict(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 80 + 4 * 16
    seen = set()
    for line in lines:
        m = re.match(r"(\d+) x (\d+) mode (\d+) nt (\d+) strength (\d+) bleed (\d+) filters (\d): equal attempts (\d+) loop (\d+) calls (\d+) differ 0 walked (\d+) fell (\d+) returned (\d+) "
                     r"loop_lanes (\d+) ns_small (\d+) fits (\d)$", line)
        assert m, line
        w, h, mode, nt, s, b, ids, att, att_loop, calls, walked, fell, back, loop_lanes, ns, fits = (int(v) for v in m.groups())
        ns_want, fit512, fit1024 = PAIRS[(s, b)]
        assert att == att_loop and ns == ns_want and fits == (fit512 if nt == 512 else fit1024), line
        assert w in WIDTHS and 4 <= h <= 6 and mode in MODES
        if ns_want == 0:
            assert calls == 0 and walked == 0 and loop_lanes == 0, line
        elif fits:
            assert calls > 0 and walked > 0 and loop_lanes == 0, line
        else:
            assert calls > 0 and walked == 0 and fell == 0 and loop_lanes > 0, line
        seen.add((s, b, nt, ids))
    assert len(seen) == len(PAIRS) * 4          # every pair at both workgroup sizes, with and without row filters


@pytest.mark.parametrize("nt", [512, 1024])
@pytest.mark.parametrize("s,b", [(19, 2), (7, 1), (15, 1)])
def test_a_lane_whose_cn_leaves_its_range_runs_the_loop_and_leaves_its_records(lib, monkeypatch, nt, s, b):
    """The engine's own error rows never push cn beyond cmax on the suite's images (the counts of the test above: no lane in the loop).  The hook's mode 2 shows the two
    bodies an incoming-error row with +-90 in two pixels of five: next to bytes near 0 or 255 the band is clamped, the diff passes the strength, cn leaves -cmax .. cmax in
    mid-segment and contracts back into the set within a few pixels.  Such lanes run the loop from their entry state; every record equals the loop's."""
    monkeypatch.setenv("SEG_HOST_ENUM_NT", str(nt))
    rng = np.random.default_rng(5)
    for img in (np.ascontiguousarray(rng.choice([0, 3, 250, 255], size=(5, 129, 4)).astype(np.uint8)), P.synth_rgba(129, 5, 5, 0)):
        want, wf = U.run_port(img, s, b)
        rc, out, f, st, cnt = run(lib, img, s, b, 2)
        rc1, out1, f1, st1, _ = run(lib, img, s, b, 1)
        assert rc == 0 and rc1 == 0 and np.array_equal(out, want) and np.array_equal(f, wf) and np.array_equal(out1, want) and int(st[0]) == int(st1[0])
        assert cnt[0] > 0 and cnt[1] == 0, cnt
        if cnt[7]:
            assert cnt[2] > 0 and cnt[3] > 0 and 0 < cnt[4] < cnt[3], cnt      # lanes that walked, lanes that ran the loop, of these: some back in the set, some not
        else:
            assert (nt, s, b) in ((1024, 19, 2), (1024, 15, 1)) and cnt[3] == 0 and cnt[5] > 0, cnt


@pytest.mark.parametrize("s,b", [(19, 2), (15, 1), (7, 1)])
@pytest.mark.parametrize("key,filters", [("r4_many_attempts_s200_b32767_null", False), ("r4_many_attempts_s255_b3_ids", True)])
def test_epochs_inside_a_row_pass_through_the_body(lib, key, filters, s, b):
    """the two tiny fixtures of the round-4 parity campaign (few counts in the histogram: rows keep failing validation and are resumed at a pixel inside the row), at pairs
    that have a small set: the body is called with start_x inside the row, workgroups in front of it return, the segment that holds it is left to seg_first_body"""
    img = U.load_npz("fuzz_regressions.npz")[key]
    want, wf = U.run_port(img, s, b, filters)
    rc, out, f, st, cnt = run(lib, img, s, b, 0, filters)
    rc1, out1, f1, st1, _ = run(lib, img, s, b, 1, filters)
    rc2, _, _, st2 = U.run_seg_host(img, s, b, filters)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and np.array_equal(out, want) and np.array_equal(out1, want) and (not filters or np.array_equal(f, wf))
    assert int(st[0]) == int(st1[0]) == int(st2[0]) and int(st[1]) == int(st1[1])
    assert cnt[0] > 0 and cnt[1] == 0 and cnt[7] == 1 and cnt[2] > 0, cnt
    assert int(st[1]) > 0, st                    # restarts: epochs that began inside a row


def test_few_colours_keep_none_alive(lib):
    """an image of the suite with few colours: candidate none is not ruled out by its bound in most rows, so its workgroups run too"""
    g = U.load_npz("suite_small.npz")
    img = np.ascontiguousarray(g["tux/in"])
    rc, out, f, st, cnt = run(lib, img, 19, 2, 0)
    rc1, _, _, st1, _ = run(lib, img, 19, 2, 1)
    assert rc == 0 and rc1 == 0 and np.array_equal(out, g["tux/out"]) and np.array_equal(f, g["tux/filters"]) and int(st[0]) == int(st1[0])
    assert cnt[1] == 0 and cnt[2] > 0 and cnt[7] == 1, cnt

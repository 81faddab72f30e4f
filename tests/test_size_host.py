"""CPU tests of the size search (no GPU compute): the rule of pngloss_amd/csrc/pl_size.h and the search arena with its scanline regions
(pl_target.h), run on the CPU under the sanitizers (tests/c/size_host.cpp) against a restatement of the rule in Python (tests/util_size.py);
the argument checks and the exported symbols where no device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_size as S


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("size_host")
    return S.build_size_host(d), d


def _table(bits):
    return "".join("1" if b else "0" for b in bits)


def test_search_rule_for_every_bound_monotone_and_random_tables(harness):
    """every M in 0..85: every monotone table (strengths >= t fit), and random non-monotone ones.  Per case the probe sequence, the chosen strength,
    reached, the probe count and the bound 1 + ceil(log2(M + 1))."""
    exe, d = harness
    rng = np.random.default_rng(23)
    cases = []
    for m in range(86):
        for t in range(m + 2):                                   # strengths >= t are accepted: t = 0 everything, t = m + 1 nothing
            cases.append((m, [s >= t for s in range(m + 1)]))
    for _ in range(400):
        m = int(rng.integers(0, 86))
        cases.append((m, list(rng.random(m + 1) < rng.random())))
    got = S.run_host(exe, d, ["S %d %s" % (m, _table(tb)) for m, tb in cases])
    reached_bound = set()
    for k, ((m, tb), line) in enumerate(zip(cases, got)):
        v = [int(x) for x in line.split()]
        chosen, reached, seq = S.py_search(m, lambda s: tb[s])
        assert v[0] == chosen and v[1] == reached and v[4:] == seq and v[2] == len(seq), (m, _table(tb), line)
        assert v[3] == S.py_probe_bound(m) and len(seq) <= v[3], (m, line)
        assert all(0 <= s <= m for s in seq) and len(set(seq)) == len(seq)       # never above M, no strength probed twice
        assert seq[0] == m and reached == int(tb[m]) and (not reached or tb[chosen])      # a reached strength was probed and accepted
        if reached:
            assert chosen == 0 or not tb[max(s for s in seq if s < chosen)]              # the probe just below the chosen one was refused
            assert 0 not in seq or all(tb[s] for s in seq[: seq.index(0)])               # 0 is probed only when every probe before it passed
        if k < sum(mm + 2 for mm in range(86)) and reached:                              # monotone: the smallest strength that fits
            assert chosen == min(s for s in range(m + 1) if tb[s])
        if len(seq) == v[3]:
            reached_bound.add(m)
    assert reached_bound == set(range(86))                       # the bound is attained for every M
    assert [S.py_probe_bound(m) for m in (0, 1, 2, 3, 4, 7, 8, 19, 40, 85, 127, 128, 255)] == [1, 2, 3, 3, 4, 4, 5, 6, 7, 8, 8, 9, 9]


def test_a_probe_with_a_status_ends_the_search_at_its_strength(harness):
    exe, d = harness
    tb = _table([s >= 12 for s in range(20)])
    seq = S.py_search(19, lambda s: s >= 12)[2]
    assert seq == [19, 9, 14, 11, 12]
    got = S.run_host(exe, d, ["F 19 %s %d" % (tb, k) for k in range(1, len(seq) + 1)])
    for k, line in enumerate(got, start=1):
        assert [int(x) for x in line.split()] == [seq[k - 1], 0, k, 1] + seq[:k], line


def test_acceptance_empty_images_groups_and_argument_checks(harness):
    exe, d = harness
    big = 2 ** 63
    got = S.run_host(exe, d, ["A 0 100 100", "A 0 101 100", "A 65 1 100", "A 0 0 0", "A 0 %d %d" % (big, big), "A 0 %d %d" % (big + 1, big),
                              "E 19", "E 0", "G 19 9 -1 19 0 9 255", "G -1 -1",
                              "C 19 0 64 8 100 0 0 0 7 0 0", "C 256 0 64 8 100", "C 19 0 64 8 0", "C 19 1 64 8 0", "C 19 1 0 0 0", "C 255 0 1 1 1",
                              "C 19 0 16384 16384 5", "C 19 0 16383 16383 5", "C 19 0 64 8 100 3 3 0"])
    assert got[:6] == ["1", "0", "0", "1", "1", "0"]
    assert got[6] == got[7] == "0 1 0 1"                         # no pixels: chosen 0, reached, no probe, finished
    assert got[8] == "0:4 9:1,5 19:0,3 255:6" and got[9] == ""
    bad = str(L.PNGLOSS_INVALID_ARGUMENT)
    assert got[10:] == ["0", bad, bad, bad, "0", "0", bad, "0", bad]          # 16384 x 16384: (4 * 16384 + 1) * 16384 > 1 GiB; 16383 x 16383 fits


def test_arena_without_scanlines_is_todays_and_the_regions_are_disjoint_and_aligned(harness):
    exe, d = harness
    shapes = [(3, 2), (0, 0), (64, 8), (257, 5), (1, 1), (0, 7), (130, 6)]
    flat = " ".join("%d %d" % s for s in shapes)
    n = len(shapes)
    up = lambda v: (v + 255) // 256 * 256
    got = S.run_host(exe, d, ["L %d %d %s" % (host, scan, flat) for host in (0, 1) for scan in (-1, 0, 1, 2)] + ["R"])
    assert got[-1] == "24 0 8 12"
    for host in (0, 1):
        old, off, probe, both = ([int(x) for x in got[host * 4 + k].split()] for k in range(4))
        assert old == off                                        # the default argument and "off" give the same layout ...
        # ... which is the one the target search has today, field by field, restated here: tables, then orig, best, best_filters[, img, filters]
        at = up(24 * 3 * n)
        want = [at]
        at = up(at + 32 * n)
        want.append(at)
        at = up(at + 64 * n)
        per = []
        for w, h in shapes:
            px, rows = w * h * 4, (h if w else 0)
            one = [at]; at = up(at + px)
            one.append(at); at = up(at + px)
            one.append(at); at = up(at + rows)
            if host:
                one.append(at); at = up(at + px)
                one.append(at); at = up(at + rows)
            else:
                one += [0, 0]
            per.append(one + [0, 0, 0, 0, 0])
        assert off == [at, 0] + want + [0] + [x for one in per for x in one]
        for scan, v in ((1, probe), (2, both)):
            total, moves, jobs, records, flags = v[:5]
            ranges = [(moves, 24 * 4 * n), (jobs, 32 * n), (records, 64 * n), (flags, 4 * n)]
            for i, (w, h) in enumerate(shapes):
                orig, best, bestf, img, filt, rows, ids, brows, bids, pitch = v[5 + 10 * i: 15 + 10 * i]
                assert pitch == ((4 * w + 15) // 16 * 16 if w * h else 0)
                frows = h if w else 0
                ranges += [(orig, w * h * 4), (best, w * h * 4), (bestf, frows), (rows, pitch * h), (ids, h if pitch else 0)]
                if host:
                    ranges += [(img, w * h * 4), (filt, frows)]
                if scan == 2:
                    ranges += [(brows, pitch * h), (bids, h if pitch else 0)]
                else:
                    assert brows == bids == 0
            assert all(a % 256 == 0 for a, _ in ranges)
            live = sorted((a, a + b) for a, b in ranges if b)
            assert all(x[1] <= y[0] for x, y in zip(live, live[1:])) and live[-1][1] <= total      # nothing overlaps, everything inside


def test_bad_targets_are_refused_without_a_device():
    lib = P.hip_lib()
    one = (C.c_uint64 * 1)(100)
    zero = (C.c_uint64 * 1)(0)
    desc = (L.ImageDesc * 1)(L.ImageDesc(None, None, 64, 8))
    host = (L.HostImage * 1)(L.HostImage(None, None, 64, 8))
    for t in (P.SizeTarget(one, 256), P.SizeTarget(zero, 19), P.SizeTarget(None, 19)):
        assert lib.pngloss_hip_optimize_batch_size(None, desc, 1, C.byref(t), 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_multi_optimize_batch_host_size(None, host, 1, C.byref(t), 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_optimize_batch_size(None, desc, 1, None, 2, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT
    assert lib.pngloss_hip_optimize_batch_size(None, desc, 1, C.byref(P.SizeTarget(one, 19)), 0, None, None, None, None) == L.PNGLOSS_INVALID_ARGUMENT


def test_both_entry_points_are_exported_and_declared():
    header = open(os.path.join(U.ROOT, "include", "pngloss_hip.h")).read()
    lib = C.CDLL(os.path.join(U.ROOT, "pngloss_amd", "csrc", "libpngloss_hip.so"))
    for name in ("pngloss_hip_optimize_batch_size", "pngloss_hip_multi_optimize_batch_host_size"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in L.ABI_SYMBOLS, name
    for name in ("pngloss_hip_size_target", "pngloss_hip_size_report"):
        assert re.search(r"\}\s*%s\s*;" % name, header), name
    assert C.sizeof(P.SizeTarget) == 16 and C.sizeof(P.SizeReport) == 32 + C.sizeof(P.Distortion)

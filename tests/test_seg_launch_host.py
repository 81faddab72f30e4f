"""The shape of a row attempt of the segment engine (pngloss_amd/csrc/pl_seg_launch.h: which kernels, grids, workgroup sizes, LDS bytes and scalar arguments --
seg_attempt_launches -- and what every workgroup of those grids does -- seg_dispatch_*) on the CPU through tests/c/seg_launch_host.cpp.

PINNED: every launch equals the arithmetic pl_seg.hip's launcher did inline before the header existed, restated here in Python (py_launches, written from
that code, not from the header; the SEG_* constants come from the header through the harness).  COVERAGE: with recording stubs in the kernel bodies' place,
the workgroups of an attempt visit every piece of work the CPU harness's own loops visited before it ran the launches (py_visits, written from those loops),
each exactly once, and nothing else.  LIMITS: what the hardware and the launcher's LDS opt-ins allow.  And the oracle-parity cases of tests/test_seg_host.py
once more with grids wider than the image (SEG_HOST_GRID_PAD): what a batch does to its narrower images."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import test_seg_host as TS
from tests import util as U

NAMES = ["NFILT", "TPARTS", "TPARTS_BATCH", "GRP", "VGRP", "VGRP_BATCH", "THREADS", "SM_CTLVAL", "SM_CTLVAL_BATCH", "NSP", "NSS", "UNIT", "UNC", "UNC_SEEDS", "UNC_SEEDS1",
         "UNC_SMALL", "UNC_SMALL1", "UNT", "SM_ENUM_UNIT", "SM_ENUM_512", "SM_ENUM_1024", "SM_ENUM_SEEDED_512", "SM_ENUM_SEEDED_1024",
         "GS", "GT", "CHAIN_THREADS", "CHAIN_THREADS_UNIT", "REPLAY_NT", "REPLAY_NT_BATCH", "SM_REPLAY", "ENUM_NT_SMALL_MAX_NSEG", "CHAIN_CAP8", "CHAIN_CAP",
         "L", "COMMIT_W", "NO_VAL_CODE", "SEED_LANES",
         "K_CTL", "K_CTL_BATCH", "K_ENUM_512", "K_ENUM_1024", "K_ENUM_SEEDED_512", "K_ENUM_SEEDED_1024", "K_ENUM_UNIT", "K_ENUM_UNIT1",
         "K_GATHER_SEEDED", "K_CHAIN", "K_CHAIN_SEEDED", "K_CHAIN_UNIT", "K_REPLAY", "K_REPLAY_BATCH", "MAX_LAUNCHES"]
CTL, POST, ENUM, ENUM_SMALL, FIRST, ENUM_SEEDED, ENUM_UNIT, GATHER, EXTREMES, CHAIN, REPLAY = range(11)      # seg_stub's body ids
FIELDS = ["max_nseg", "max_ngrp", "max_ncommit", "enum_nt", "tparts", "unit", "small_ok", "seeded", "seeds"]


class K:
    pass


def consts():
    if not hasattr(K, "NFILT"):
        out = np.zeros(64, np.int64)
        n = U.seg_launch_host_lib().seg_launch_host_constants(out.ctypes.data)
        assert n == len(NAMES)
        for name, v in zip(NAMES, out[:n]):
            setattr(K, name, int(v))
    return K


def sm_chain(n, x):
    return int(U.seg_launch_host_lib().seg_launch_host_sm_chain(n, int(x)))


def cdiv(a, b):
    return (a + b - 1) // b


def c_launches(shape):
    s = np.array([int(shape[f]) for f in FIELDS], np.int64)
    out = np.zeros((8, 7), np.int64)
    n = U.seg_launch_host_lib().seg_launch_host_launches(s.ctypes.data, out.ctypes.data)
    return [tuple(int(x) for x in r) for r in out[:n]]


def py_launches(b):
    """pl_seg_launch_attempt() as pl_seg.hip had it: (kernel, grid_x, threads, lds_bytes, a, b, seeds) per launch; scalar arguments a kernel does not take are 0"""
    k = consts()
    out = []
    vgrp = k.VGRP_BATCH if b["tparts"] == k.TPARTS_BATCH else k.VGRP
    nctl = k.NFILT * b["tparts"] + 1 + b["max_ncommit"]
    nval = 0 if k.NO_VAL_CODE else k.NFILT * b["max_ngrp"] * (k.GRP // vgrp)
    if b["tparts"] == k.TPARTS_BATCH:
        out.append((k.K_CTL_BATCH, nctl + nval, k.THREADS, k.SM_CTLVAL_BATCH, nctl, b["max_ngrp"], 0))
    else:
        out.append((k.K_CTL, nctl + nval, k.THREADS, k.SM_CTLVAL, nctl, b["max_ngrp"], 0))
    small_ok, nt, nseg = b["small_ok"], b["enum_nt"], b["max_nseg"]
    halves, small_segs = 4 // (nt // k.NSP), nt // (4 * k.NSS)
    blocks = (3 * nseg * halves + 2 * cdiv(nseg, small_segs) if small_ok else k.NFILT * nseg * halves) + k.NFILT
    if b["unit"] == 1 and b["seeds"] and not b["seeded"]:
        pairs, nc_min = nseg * 4, min(k.UNC_SEEDS1, k.UNC)
        perb, pers = cdiv(pairs, nc_min), cdiv(pairs, k.UNC_SMALL1)
        out.append((k.K_ENUM_UNIT1, (3 * perb + 2 * pers if small_ok else k.NFILT * perb) + k.NFILT, k.UNT, k.SM_ENUM_UNIT, perb, pers, 1))
    elif b["unit"] > 1 and not b["seeded"]:
        pairs = cdiv(nseg, k.UNIT) * 4
        nc_min = k.UNC_SEEDS if b["seeds"] and k.UNC_SEEDS < k.UNC else k.UNC
        perb, pers = cdiv(pairs, nc_min), cdiv(pairs, k.UNC_SMALL)
        out.append((k.K_ENUM_UNIT, (3 * perb + 2 * pers if small_ok else k.NFILT * perb) + k.NFILT, k.UNT, k.SM_ENUM_UNIT, perb, pers, 1 if b["seeds"] else 0))
    elif b["seeded"]:
        sblocks = k.NFILT * nseg * halves + k.NFILT
        if nt == 512:
            out.append((k.K_ENUM_SEEDED_512, sblocks, 512, k.SM_ENUM_SEEDED_512, nseg, 0, 0))
        else:
            out.append((k.K_ENUM_SEEDED_1024, sblocks, 1024, k.SM_ENUM_SEEDED_1024, nseg, 0, 0))
    elif nt == 512:
        out.append((k.K_ENUM_512, blocks, 512, k.SM_ENUM_512, nseg, 0, 0))
    else:
        out.append((k.K_ENUM_1024, blocks, 1024, k.SM_ENUM_1024, nseg, 0, 0))
    if b["seeded"] and nseg > 1:
        nblk = cdiv(nseg - 1, k.GS)
        out.append((k.K_GATHER_SEEDED, k.NFILT * 4 * nblk, k.GT, 0, nblk, 0, 0))
    if b["seeded"]:
        out.append((k.K_CHAIN_SEEDED, k.NFILT * 4 + 1, k.CHAIN_THREADS, sm_chain(nseg, False), 0, 0, 0))
    elif b["unit"] > 1:
        out.append((k.K_CHAIN_UNIT, k.NFILT * 4 + 1, k.CHAIN_THREADS_UNIT, sm_chain(cdiv(nseg, b["unit"]), True), 0, 0, 0))
    else:
        out.append((k.K_CHAIN, k.NFILT * 4 + 1, k.CHAIN_THREADS, sm_chain(nseg, True), 0, 0, 0))
    if b["unit"] > 1:
        out.append((k.K_REPLAY_BATCH, k.NFILT * b["max_ngrp"], k.REPLAY_NT_BATCH, k.SM_REPLAY, b["max_ngrp"], 0, 0))
    else:
        out.append((k.K_REPLAY, k.NFILT * b["max_ngrp"], k.REPLAY_NT, k.SM_REPLAY, b["max_ngrp"], 0, 0))
    return out


def make_shape(max_nseg, enum_nt, tparts, unit, small_ok, seeded, seeds, width=None):
    k = consts()
    width = max_nseg * k.L if width is None else width
    assert cdiv(width, k.L) == max_nseg
    return dict(max_nseg=max_nseg, max_ngrp=cdiv(max_nseg, k.GRP), max_ncommit=cdiv(width, k.COMMIT_W), enum_nt=enum_nt, tparts=tparts, unit=unit,
                small_ok=small_ok, seeded=seeded, seeds=seeds)


def shapes(rng, count):
    """the shapes pl_plan_batch can produce: seeded state sets are enumerated per segment and never from seeds; everything else combines (the hooks pin
    enum_nt and tparts independently of the rest)"""
    k = consts()
    edge = [1, 2, k.ENUM_NT_SMALL_MAX_NSEG - 1, k.ENUM_NT_SMALL_MAX_NSEG, k.ENUM_NT_SMALL_MAX_NSEG + 1, k.CHAIN_CAP8, k.CHAIN_CAP + 1, 32768]
    combos = [(nt, tp, unit, small_ok, seeded, seeds) for nt in (512, 1024) for tp in (k.TPARTS, k.TPARTS_BATCH) for unit in (1, k.UNIT) for small_ok in (False, True)
              for seeded in (False, True) for seeds in (False, True) if not (seeded and (unit > 1 or seeds))]
    out = [make_shape(n, *c) for n in edge for c in combos]
    for _ in range(count):
        n = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(1, 700)), int(rng.integers(1, 32769))]))
        c = combos[int(rng.integers(0, len(combos)))]
        out.append(make_shape(n, *c, width=n * k.L - int(rng.integers(0, k.L))))
    return out


def test_launches_are_the_parents_arithmetic():
    rng = np.random.default_rng(21)
    all_shapes = shapes(rng, 400)
    kernels = set()
    for b in all_shapes:
        got = c_launches(b)
        assert got == py_launches(b), b
        kernels.update(g[0] for g in got)
    k = consts()
    assert kernels == {getattr(k, n) for n in NAMES if n.startswith("K_")}              # every kernel of the library is launched by some shape


def test_launch_limits():
    k = consts()
    rng = np.random.default_rng(22)
    opted_in = {k.K_CHAIN, k.K_CHAIN_SEEDED, k.K_CHAIN_UNIT, k.K_CTL, k.K_CTL_BATCH}       # pl_seg.hip:chain_attr (the control kernels when they ask for more than 64 KB)
    for b in shapes(rng, 400):
        got = c_launches(b)
        gather = b["seeded"] and b["max_nseg"] > 1
        assert len(got) == (5 if gather else 4) and len(got) <= k.MAX_LAUNCHES, b
        assert (k.K_GATHER_SEEDED in [g[0] for g in got]) == gather
        for kernel, grid_x, threads, lds, *_ in got:
            assert 0 < grid_x < 2 ** 31 and 0 < threads <= 1024 and 0 <= lds <= 160 * 1024, (b, kernel)
            assert kernel in opted_in or lds <= 65536, (b, kernel)


def prev(par):
    return 2 if par == 0 else par - 1


def py_visits(b, launches, par, W, bpp, seed_n, nbreak, y, start_x):
    """what the CPU harness's own loops over an attempt visited (tests/c/seg_host.cpp before it ran the library's launches), plus the control launch's
    workgroups: (launch, body, template arguments, par, arguments)"""
    k = consts()
    nseg = cdiv(W, k.L)
    ngrp = cdiv(nseg, k.GRP)
    small = lambda f: b["small_ok"] and f in (0, 2)
    from_seeds = lambda f: bool(b["seeds"]) and seed_n > 0 and not small(f) and start_x[f] == 0 and nbreak * 16 <= y + 128      # seg_unit_from_seeds
    out = []
    for li, (kernel, *_rest) in enumerate(launches):
        if kernel in (k.K_CTL, k.K_CTL_BATCH):
            tp, vgrp = (k.TPARTS, k.VGRP) if kernel == k.K_CTL else (k.TPARTS_BATCH, k.VGRP_BATCH)
            assert tp == b["tparts"]
            out += [(li, CTL, tp, 0, par, bx, 0, 0) for bx in range(k.NFILT * tp + 1 + cdiv(W, k.COMMIT_W))]
            if not k.NO_VAL_CODE:
                out += [(li, POST, vgrp, 0, prev(par), f, vg, 0) for f in range(k.NFILT) for vg in range(cdiv(nseg, vgrp))]
        elif kernel in (k.K_ENUM_512, k.K_ENUM_1024):
            nt = 512 if kernel == k.K_ENUM_512 else 1024
            for f in range(k.NFILT):
                if small(f):
                    out += [(li, ENUM_SMALL, nt, 0, par, f, sg, 0) for sg in range(0, nseg, nt // 128)]
                else:
                    out += [(li, ENUM, nt, 0, par, f, sg, ch) for sg in range(nseg) for ch in range(1024 // nt)]
            out += [(li, FIRST, nt, 0, par, f, 0, 0) for f in range(k.NFILT)]
        elif kernel in (k.K_ENUM_SEEDED_512, k.K_ENUM_SEEDED_1024):
            nt = 512 if kernel == k.K_ENUM_SEEDED_512 else 1024
            out += [(li, ENUM_SEEDED, nt, 0, par, f, sg, ch) for f in range(k.NFILT) for sg in range(nseg) for ch in range(1024 // nt)]
            out += [(li, FIRST, nt, 0, par, f, 0, 0) for f in range(k.NFILT)]
        elif kernel in (k.K_ENUM_UNIT, k.K_ENUM_UNIT1):
            u = k.UNIT if kernel == k.K_ENUM_UNIT else 1
            npairs = cdiv(nseg, u) * bpp
            for f in range(k.NFILT):
                if small(f):
                    lanes, nc, sd = k.NSS, (k.UNC_SMALL if u == k.UNIT else k.UNC_SMALL1), 0
                elif from_seeds(f):
                    lanes, nc, sd = k.SEED_LANES, (k.UNC_SEEDS1 if u == 1 else k.UNC_SEEDS), 1
                else:
                    lanes, nc, sd = k.NSP, k.UNC, 0
                out += [(li, ENUM_UNIT, lanes, (u * 1000 + nc) * 2 + sd, par, f, g, 0) for g in range(cdiv(npairs, nc))]
            out += [(li, FIRST, k.UNT, int(u > 1), par, f, 0, 0) for f in range(k.NFILT)]
        elif kernel == k.K_GATHER_SEEDED:
            if nseg > 1:
                out += [(li, GATHER, 0, 0, -1, f, c, blk) for f in range(k.NFILT) for c in range(4) for blk in range(cdiv(nseg - 1, k.GS))]
        elif kernel in (k.K_CHAIN, k.K_CHAIN_SEEDED, k.K_CHAIN_UNIT):
            ct, t1 = {k.K_CHAIN: (k.CHAIN_THREADS, 0), k.K_CHAIN_SEEDED: (k.CHAIN_THREADS, 2), k.K_CHAIN_UNIT: (k.CHAIN_THREADS_UNIT, 1)}[kernel]
            out.append((li, EXTREMES, ct, 0, par, 0, 0, 0))
            out += [(li, CHAIN, ct, t1, par, f, c, 0) for f in range(k.NFILT) for c in range(4)]
        elif kernel in (k.K_REPLAY, k.K_REPLAY_BATCH):
            rnt = k.REPLAY_NT if kernel == k.K_REPLAY else k.REPLAY_NT_BATCH
            out += [(li, REPLAY, rnt, 0, par, f, g, 0) for f in range(k.NFILT) for g in range(ngrp)]
        else:
            raise AssertionError("a kernel this test cannot classify: %r of %r" % (kernel, b))
    return out


def c_visits(b, par, W, bpp, seed_n, nbreak, y, start_x):
    s = np.array([int(b[f]) for f in FIELDS], np.int64)
    img = np.array([W, bpp, seed_n, nbreak, y] + list(start_x), np.int64)
    cap = 1 << 16
    while True:
        out = np.zeros((cap, 8), np.int32)
        n = int(U.seg_launch_host_lib().seg_launch_host_visit(s.ctypes.data, par, img.ctypes.data, out.ctypes.data, cap))
        if n <= cap:
            return [tuple(int(x) for x in r) for r in out[:n]]
        cap = n


def test_every_piece_of_work_is_visited_exactly_once():
    k = consts()
    rng = np.random.default_rng(23)
    all_shapes = [b for b in shapes(rng, 250) if b["max_nseg"] <= 2200]          # (the widest rows: a few, below)
    all_shapes += [make_shape(32768, 512, k.TPARTS, 1, True, False, False), make_shape(32768, 1024, k.TPARTS_BATCH, k.UNIT, True, False, True),
                   make_shape(20000, 1024, k.TPARTS, 1, False, True, False)]
    bodies = set()
    for i, b in enumerate(all_shapes):
        launches = py_launches(b)
        top = b["max_nseg"] * k.L
        # an image of the group: the widest itself with and without a partial last segment, one a few segments narrower (idle workgroups in every grid), a tiny one
        widths = {top, max(top - 5, top - k.L + 1), max(1, top - int(rng.integers(0, 40)) * k.L - int(rng.integers(0, k.L))), int(rng.integers(1, 70))}
        for W in sorted(w for w in widths if cdiv(w, k.L) <= b["max_nseg"] and cdiv(w, k.COMMIT_W) <= b["max_ncommit"]):
            bpp, par = 1 + (i + W) % 4, int(rng.integers(0, 3))
            seed_n = int(rng.choice([0, 47]))
            nbreak, y = int(rng.choice([0, 0, 3, 40])), int(rng.integers(0, 300))
            start_x = [int(rng.choice([0, 0, 33])) for _ in range(k.NFILT)]
            got = c_visits(b, par, W, bpp, seed_n, nbreak, y, start_x)
            want = py_visits(b, launches, par, W, bpp, seed_n, nbreak, y, start_x)
            assert len(got) == len(set(got)), (b, W)                    # nothing twice
            assert sorted(got) == sorted(want), (b, W, bpp, seed_n, nbreak, y, start_x)
            bodies.update((g[1], g[2], g[3]) for g in got)
    assert {g[0] for g in bodies} == set(range(11))
    assert {(ENUM_UNIT, k.SEED_LANES, (u * 1000 + nc) * 2 + 1) for u, nc in ((1, k.UNC_SEEDS1), (k.UNIT, k.UNC_SEEDS))} <= bodies      # both starts from seeds ran


# ------------------------------------------------------------------------------------------------ grids wider than the image, through the real bodies

PADS = (1, 9, 17)


def test_the_pads_cross_a_commit_workgroup_and_a_replay_group():
    k = consts()
    assert any(p * k.L > k.COMMIT_W for p in PADS) and any(p > k.GRP for p in PADS) and 1 in PADS


def padded_matches_oracle(monkeypatch, w, h, mode, s, b):
    img = P.synth_rgba(w, h, mode, 0)
    want, wf = U.run_port(img, s, b)
    for pad in PADS:
        monkeypatch.setenv("SEG_HOST_GRID_PAD", str(pad))
        rc, out, f, st = U.run_seg_host(img, s, b)
        assert rc == 0 and np.array_equal(out, want) and np.array_equal(f, wf), pad


@pytest.mark.parametrize("w,h,mode,s,b", TS.CASES)
def test_padded_grids_bodies_match_oracle(monkeypatch, w, h, mode, s, b):
    padded_matches_oracle(monkeypatch, w, h, mode, s, b)


@pytest.mark.parametrize("w,h,mode,s,b", TS.UNIT_CASES)
def test_padded_grids_enumeration_in_units_matches_oracle(monkeypatch, w, h, mode, s, b):
    monkeypatch.setenv("SEG_HOST_UNIT", "1")
    padded_matches_oracle(monkeypatch, w, h, mode, s, b)


@pytest.mark.parametrize("w,h,mode,s,b", TS.UNIT_CASES + [(1920, 24, 0, 19, 2), (700, 30, 1, 19, 2), (513, 20, 5, 19, 2), (900, 16, 0, 12, 1), (1600, 10, 0, 7, 3), (640, 12, 0, 31, 8)])
def test_padded_grids_units_from_seeds_match_oracle(monkeypatch, w, h, mode, s, b):
    monkeypatch.setenv("SEG_HOST_UNIT", "1")
    monkeypatch.setenv("SEG_HOST_SEEDS", "1")
    padded_matches_oracle(monkeypatch, w, h, mode, s, b)


@pytest.mark.parametrize("w,h,mode,s,b", [(1024, 24, 0, 19, 2), (700, 30, 1, 19, 2), (513, 20, 5, 19, 2), (385, 20, 2, 19, 2), (289, 20, 3, 19, 2), (193, 20, 4, 19, 2), (95, 7, 0, 19, 2),
                                          (33, 9, 1, 19, 2), (1600, 10, 0, 7, 3), (900, 16, 0, 12, 1), (640, 12, 0, 31, 8), (2100, 5, 0, 19, 2)])
def test_padded_grids_segments_from_seeds_match_oracle(monkeypatch, w, h, mode, s, b):
    monkeypatch.setenv("SEG_HOST_UNIT", "0")
    monkeypatch.setenv("SEG_HOST_SEEDS", "1")
    padded_matches_oracle(monkeypatch, w, h, mode, s, b)

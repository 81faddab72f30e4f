"""GPU tests of pngloss_hip_optimize_batch_size and its host form: the strength the library finds for a byte budget is the one the rule gives on the
CPU chain (tests/golden/size_target_table.json), the image then holds what a plain batch at that strength writes, and the size it reports is the
size of the stream the writing deflate produces.  Equality is exact everywhere."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_size as S
from tests import util_target as T

pytestmark = pytest.mark.gpu

HUGE = 2 ** 63
REFERENCE_FIELDS = ("status", "bpp", "unique_symbols", "retried_rows")


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C").reshape(-1)).cuda()


def _device_batch(imgs):
    import torch
    dev = [_dev(a) for a in imgs]
    flt = [torch.zeros(max(a.shape[0], 1), dtype=torch.uint8, device="cuda") for a in imgs]
    desc = [(d.data_ptr() if a.size else 0, f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)]
    return dev, flt, desc


def _back(dev, flt, imgs):
    import torch
    torch.cuda.synchronize()
    return [d.cpu().numpy().reshape(a.shape) for d, a in zip(dev, imgs)], [f.cpu().numpy()[: a.shape[0]] for f, a in zip(flt, imgs)]


def _cases_by_m():
    out = {}
    for c in S.load_table()["cases"]:
        out.setdefault(c["M"], []).append(c)
    return out


@pytest.mark.parametrize("engine", ["seg", "wg"])
@pytest.mark.parametrize("m", sorted(_cases_by_m()))
def test_device_form_against_the_table(m, engine):
    """every case of the table with this M in ONE call (a call has one M, budgets are per image): strength, reached, probes, runs and bytes equal the
    table; pixels and row filters equal a plain batch at the chosen strength."""
    cases = _cases_by_m()[m]
    imgs = [T.oracle_probe(*c["shape"], 0)[0] for c in cases]
    ctx = P.HipContext()
    try:
        ctx.set_option("engine", engine)
        dev, flt, desc = _device_batch(imgs)
        res, rep, _ = ctx.run_size(desc, [c["budget"] for c in cases], m, S.BLEED)
        outs, filts = _back(dev, flt, imgs)
        plain_of = {}
        for i, c in enumerate(cases):
            got = (rep[i].strength, rep[i].reached, rep[i].probes, rep[i].runs, rep[i].bytes, rep[i].color_type)
            assert got == (c["chosen"], c["reached"], len(c["probes"]), len(c["probes"]), c["bytes"], c["color_type"]), (c, rep[i].as_dict())
            key = (tuple(c["shape"]), c["chosen"])
            if key not in plain_of:
                pdev, pflt, pdesc = _device_batch([imgs[i]])
                plain = ctx.run(pdesc, c["chosen"], S.BLEED)
                pouts, pfilts = _back(pdev, pflt, [imgs[i]])
                plain_of[key] = (pouts[0], pfilts[0], plain[0])
            pout, pfilt, pres = plain_of[key]
            assert np.array_equal(outs[i], pout) and np.array_equal(filts[i], pfilt), c
            assert {k: res[i][k] for k in REFERENCE_FIELDS} == {k: pres[k] for k in REFERENCE_FIELDS}, c
            _, want, want_f, want_rec, _ = T.oracle_probe(*c["shape"], c["chosen"])
            assert np.array_equal(outs[i], want) and np.array_equal(filts[i], want_f) and rep[i].distortion.as_dict() == want_rec, c
    finally:
        ctx.close()


def test_report_size_is_the_stream_and_the_stream_is_host_zlibs():
    """independent of the oracle: reports[i].bytes == streams[i].size, the stream inflates to the scanlines _host_emit returns at that strength and
    equals the _host_zlib stream at that strength byte for byte"""
    cases = [c for c in _cases_by_m()[19] if c["outcome"] in ("interior", "only_at_M", "unreachable", "at_0")]
    picked, seen = [], set()
    for c in cases:                                              # one case per (shape, outcome)
        if (tuple(c["shape"]), c["outcome"]) not in seen:
            seen.add((tuple(c["shape"]), c["outcome"]))
            picked.append(c)
    imgs = [T.oracle_probe(*c["shape"], 0)[0] for c in picked]
    ctx = P.HipContext()
    try:
        dev, flt, desc = _device_batch(imgs)
        res, rep, streams = ctx.run_size(desc, [c["budget"] for c in picked], 19, S.BLEED, want_streams=True)
        for i, c in enumerate(picked):
            ctype, z, blocks = streams[i]
            assert rep[i].bytes == len(z) and rep[i].strength == c["chosen"] and rep[i].runs == rep[i].probes, (c, rep[i].as_dict())
            assert not rep[i].reached or len(z) <= c["budget"]
            _, _, emitted = ctx.run_host_emit([imgs[i]], rep[i].strength, S.BLEED)
            ectype, ids, rows = emitted[0]
            assert ctype == ectype == rep[i].color_type
            assert zlib.decompress(z) == b"".join(bytes([int(t)]) + r.tobytes() for t, r in zip(ids, rows)), c
            _, _, hz = ctx.run_host_zlib([imgs[i]], rep[i].strength, S.BLEED)
            assert hz[0][1] == z and tuple(hz[0][2]) == tuple(blocks), c
    finally:
        ctx.close()


def _measure_batch():
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    const = np.full((30, 70, 4), 200, np.uint8)
    return [T.oracle_probe(1, 1, 0, 0)[0], T.oracle_probe(1, 300, 0, 0)[0], np.zeros((0, 0, 4), np.uint8), const, noise, T.oracle_probe(300, 300, 0, 0)[0]]


def check_measure_against_writing_mode():
    """the measure-only deflate against the writing one, both through the public calls, M = 19.  A budget of 2^63 is met by every strength, so the rule
    walks down to strength 0 (probes 19, 9, 4, 1, 0): the reported size is compared with _host_zlib at the reported strength.  A budget of 1 byte is
    met by none: one probe, the image keeps the M result, and the reported size is the measured size at 19, compared with _host_zlib at 19."""
    imgs = _measure_batch()
    ctx = P.HipContext()
    try:
        kinds = set()
        for budget, strength, probes, reached in ((HUGE, 0, 5, 1), (1, 19, 1, 0)):
            dev, flt, desc = _device_batch(imgs)
            res, rep, streams = ctx.run_size(desc, [budget] * len(imgs), 19, S.BLEED, want_streams=True)
            _, _, hz = ctx.run_host_zlib(imgs, strength, S.BLEED)
            for i, a in enumerate(imgs):
                want = (strength, probes, probes, reached) if a.size else (0, 0, 0, 1)
                assert (rep[i].strength, rep[i].probes, rep[i].runs, rep[i].reached) == want, (budget, i, rep[i].as_dict())
                assert rep[i].bytes == len(hz[i][1]) == len(streams[i][1]) and streams[i][1] == hz[i][1] and streams[i][2] == tuple(hz[i][2]), (budget, i)
                assert (rep[i].bytes == 0) == (a.size == 0)
                for k in range(3):
                    if hz[i][2][k]:
                        kinds.add(k)
            assert sum(hz[5][2]) == 2                            # the two-block image
        assert 0 in kinds and 2 in kinds                         # stored (noise) and dynamic blocks were measured
    finally:
        ctx.close()


def test_measure_only_against_writing_mode():
    check_measure_against_writing_mode()


def test_measure_only_against_writing_mode_in_several_groups():
    """again with PNGLOSS_HIP_DEFLATE_GROUP_BYTES set small, in a fresh child process: both deflates run the batch as several groups"""
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_size as G; G.check_measure_against_writing_mode(); print('groups ok')" % U.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=U.ROOT,
                       env=dict(os.environ, PNGLOSS_HIP_DEFLATE_GROUP_BYTES="2000", PNGLOSS_HIP_DEBUG="1"))
    assert r.returncode == 0 and "groups ok" in r.stdout, r.stderr[-3000:]
    assert r.stderr.count("pngloss_hip deflate (measure only):") >= 3, r.stderr[-3000:]      # 1 x 300 and 1 x 1 share a group, the others have their own


def test_host_form_on_two_contexts():
    cases = []
    seen = set()
    for c in _cases_by_m()[19]:
        if (tuple(c["shape"]), c["outcome"]) not in seen and c["shape"] != [300, 300, 0]:
            seen.add((tuple(c["shape"]), c["outcome"]))
            cases.append(c)
    big = next(c for c in _cases_by_m()[19] if c["shape"] == [300, 300, 0] and c["outcome"] == "interior")
    cases.append(big)
    imgs = [T.oracle_probe(*c["shape"], 0)[0] for c in cases] + [np.zeros((0, 0, 4), np.uint8)]
    budgets = [c["budget"] for c in cases] + [0]
    multi = P.HipMulti("0,0")
    try:
        assert multi.count == 2
        multi.set_option("distortion", "on")
        outs, filts, res, rep, scan, streams = multi.run_host_size(imgs, budgets, 19, S.BLEED, emit="both")
        with pytest.raises(RuntimeError):
            multi.distortion(0)                                  # the _last_* accessors refuse: the records are in the reports
        with pytest.raises(RuntimeError):
            multi.ssim(0)
        assert len({r.strength for r in rep}) >= 3
        for i, c in enumerate(cases):
            assert (rep[i].strength, rep[i].reached, rep[i].probes, rep[i].bytes) == (c["chosen"], c["reached"], len(c["probes"]), c["bytes"]), (c, rep[i].as_dict())
            assert rep[i].runs == rep[i].probes + 1
            assert rep[i].bytes == len(streams[i][1]) and (not rep[i].reached or len(streams[i][1]) <= budgets[i])
            assert rep[i].distortion.as_dict() == T.oracle_probe(*c["shape"], c["chosen"])[3]
        assert (rep[-1].strength, rep[-1].probes, rep[-1].runs, rep[-1].reached, rep[-1].bytes) == (0, 0, 0, 1, 0)
        # the plain multi call at the reported strengths: the same outputs, image by image
        for strength in sorted({r.strength for r in rep[:-1]}):
            who = [i for i in range(len(cases)) if rep[i].strength == strength]
            pouts, pfilts, pres = multi.run_host([imgs[i] for i in who], strength, S.BLEED)
            for k, i in enumerate(who):
                assert np.array_equal(outs[i], pouts[k]) and np.array_equal(filts[i], pfilts[k]) and res[i]["status"] == pres[k]["status"] == 0, cases[i]
        # "distortion" is left as the caller set it: the next plain multi batch is measured
        assert multi.distortion(0).as_dict() == T.oracle_probe(*cases[who[0]]["shape"], strength)[3]
        ctx = P.HipContext()
        try:
            for i, c in enumerate(cases):
                _, _, em = ctx.run_host_emit([imgs[i]], rep[i].strength, S.BLEED)
                assert scan[i][0] == em[0][0] == streams[i][0] and np.array_equal(scan[i][1], em[0][1]) and np.array_equal(scan[i][2], em[0][2]), c
                assert zlib.decompress(streams[i][1]) == b"".join(bytes([int(t)]) + r.tobytes() for t, r in zip(em[0][1], em[0][2])), c
        finally:
            ctx.close()
    finally:
        multi.close()


def test_context_afterwards_and_the_callers_options():
    lib = P.hip_lib()
    c = next(c for c in _cases_by_m()[19] if c["shape"] == [64, 16, 0] and c["outcome"] == "interior")
    img = T.oracle_probe(*c["shape"], 0)[0]
    ctx = P.HipContext()
    try:
        ctx.set_option("distortion", "on")
        dev, flt, desc = _device_batch([img])
        res, rep, _ = ctx.run_size(desc, [c["budget"]], 19, S.BLEED)
        assert rep[0].strength == c["chosen"]
        out, sout, hist = P.Distortion(), P.Ssim(), np.zeros(256, np.uint32)
        assert lib.pngloss_hip_last_distortion(ctx._ctx, 0, out) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_last_ssim(ctx._ctx, 0, sout) == L.PNGLOSS_INVALID_ARGUMENT
        assert lib.pngloss_hip_last_histogram(ctx._ctx, 0, hist.ctypes.data_as(L.C.c_void_p)) == L.PNGLOSS_INVALID_ARGUMENT
        # the option is still on: the next plain batch is measured
        pdev, pflt, pdesc = _device_batch([img])
        assert ctx.run(pdesc, 19, S.BLEED)[0]["status"] == 0
        assert ctx.distortion(0).as_dict() == T.oracle_probe(*c["shape"], 19)[3]
        assert ctx.run_size([], [], 19, S.BLEED) == ([], [], None)
    finally:
        ctx.close()


OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers on this box)")
def test_tool_fits_files_into_their_budgets(tmp_path):
    """three small PNGs with --target-size 40%, with an absolute budget and with a budget below the container size: every written file is at most
    its budget, or the warning line is there and the file equals --gpu-deflate -s M; each file equals --gpu-deflate -s <chosen> byte for byte"""
    import re
    from PIL import Image
    shapes = [(64, 16, 0), (130, 6, 3), (33, 16, 2)]
    names = ["a", "b", "c"]
    M = 19
    src = tmp_path / "src"
    src.mkdir()
    for n, (w, h, mode) in zip(names, shapes):
        Image.fromarray(T.oracle_probe(w, h, mode, 0)[0], "RGBA").save(src / f"{n}.png")

    def run(tag, args, files):
        d = tmp_path / tag
        d.mkdir()
        for n in files:
            (d / f"{n}.png").write_bytes((src / f"{n}.png").read_bytes())
        r = subprocess.run([OUR_CLI] + args + [str(d / f"{n}.png") for n in files], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stderr[-800:])
        return [(d / f"{n}-loss.png").read_bytes() for n in files], r.stderr.splitlines(), d

    plain = {}

    def plain_at(n, strength):
        if (n, strength) not in plain:
            plain[(n, strength)] = run(f"plain_{n}_{strength}", ["--gpu-deflate", "-s", str(strength)], [n])[0][0]
        return plain[(n, strength)]

    outcomes = set()
    for tag, value, budget_of in (("percent", "40%", lambda size: max(1, size * 40 // 100)), ("absolute", "1000", lambda size: 1000),
                                  ("suffix", "1k", lambda size: 1024), ("below_container", "50", lambda size: 50)):
        got, err, d = run(tag, ["--target-size", value, "-s", str(M), "-v"], names)
        chosen = [tuple(map(int, re.match(r"  strength (\d+) chosen in (\d+) probes", x).groups())) for x in err if x.startswith("  strength ")]
        assert len(chosen) == 3, err
        for n, data, (strength, probes) in zip(names, got, chosen):
            budget = budget_of(len((src / f"{n}.png").read_bytes()))
            warned = [x for x in err if x.startswith("  warning: ") and f"/{n}.png" in x]
            assert 1 <= probes <= S.py_probe_bound(M) and 0 <= strength <= M
            if len(data) <= budget:
                assert not warned, (tag, n, warned)
                outcomes.add("fits at M" if strength == M else "fits below M")
            else:
                assert len(warned) == 1 and ("budget of %d bytes" % budget) in warned[0] and ("wrote %d bytes" % len(data)) in warned[0], (tag, n, err)
                assert strength == M and probes == 1 and data == plain_at(n, M), (tag, n)
                outcomes.add("warned")
            assert data == plain_at(n, strength), (tag, n, strength)
            if strength > 0 and len(data) <= budget and probes > 1:
                assert len(plain_at(n, strength)) <= budget          # (what the search kept is what a plain run at that strength writes)
        if tag == "below_container":
            assert sum(1 for x in err if x.startswith("  warning: ")) == 3
    assert {"warned", "fits below M"} <= outcomes, outcomes
    # the switch goes with the reporting and path switches of --gpu-deflate
    got2, err2, _ = run("with_reports", ["--target-size", "1000", "-s", str(M), "-v", "--gpu-read", "--distortion"], names)
    got1, _, _ = run("again", ["--target-size", "1000", "-s", str(M)], names)
    assert got2 == got1 and sum(1 for x in err2 if x.startswith("  distortion:")) == 3

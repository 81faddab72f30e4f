"""GPU side of tests/test_seg_kernarg_host.py (-m gpu): the segment engine, pinned, with its kernels' arguments preloaded and the replay's record and view
requested in one burst, against the CPU oracle bit for bit (bytes and filter ids) at the shapes where a kernel's head decides something: one segment
(width 1, 32), a partial second segment (33), a second replay group and a third commit workgroup (513), heights 3-4; an exhaustive state set (s=19 b=2)
and the seeded five-launch attempt (s=85 b=1); a batch of three images of different widths, one of them empty (record index > 0, idle workgroups); the
two fixtures that need very many attempts (epochs, void attempts, failed validations that an attempt ignores or does not).  For single images the
device takes exactly the attempts that the CPU harness (tests/c/seg_host.cpp) takes for the same input: the harness reports the number of the attempt whose
control launch found the image finished, the device's result record the attempt in front of that one (pl_seg_core.h: seg_ctl_body writes cur.attempts), so the two
differ by that one launch."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu

WIDTHS = (1, 32, 33, 513)
HEIGHTS = (3, 4)
PAIRS = ((19, 2), (85, 1))


@pytest.fixture()
def seg_ctx(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    ctx = P.HipContext()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("s,b", PAIRS)
@pytest.mark.parametrize("w", WIDTHS)
def test_single_images_match_oracle_in_the_harness_attempts(seg_ctx, w, s, b):
    for h in HEIGHTS:
        img = P.synth_rgba(w, h, 0, w + h)
        want, wf = U.run_port(img, s, b)
        rc, host_out, host_f, st = U.run_seg_host(img, s, b)
        assert rc == 0 and np.array_equal(host_out, want) and np.array_equal(host_f, wf), (w, h, s, b)
        (out,), (f,), res = seg_ctx.run_host([img], s, b)
        info = seg_ctx.engine_info(0)
        assert res[0]["status"] == 0 and info["engine"] == "segment-parallel", (w, h, s, b, info)
        assert np.array_equal(out, want) and np.array_equal(f, wf), (w, h, s, b)
        assert info["attempts"] + 1 == int(st[0]), (w, h, s, b, info, st)


@pytest.mark.parametrize("s,b", PAIRS)
def test_a_batch_of_three_widths_one_image_empty(seg_ctx, s, b):
    imgs = [P.synth_rgba(513, 4, 0, 1), np.zeros((0, 0, 4), np.uint8), P.synth_rgba(33, 3, 5, 2)]
    outs, filts, res = seg_ctx.run_host(imgs, s, b)
    for i, (img, out, f, r) in enumerate(zip(imgs, outs, filts, res)):
        assert r["status"] == 0, (i, s, b, r)
        if img.size == 0:
            assert out.size == 0
            continue
        want, wf = U.run_port(img, s, b)
        assert seg_ctx.engine_info(i)["engine"] == "segment-parallel"
        assert np.array_equal(out, want) and np.array_equal(f, wf), (i, s, b)


@pytest.mark.parametrize("key,s,b,filters", [("r4_many_attempts_s200_b32767_null", 200, 32767, False), ("r4_many_attempts_s255_b3_ids", 255, 3, True)])
def test_images_that_need_very_many_attempts(seg_ctx, key, s, b, filters):
    img = U.load_npz("fuzz_regressions.npz")[key]
    want, wf = U.run_port(img, s, b, filters)
    rc, _, _, st = U.run_seg_host(img, s, b, filters)
    (out,), (f,), res = seg_ctx.run_host([img], s, b, want_filters=filters)
    info = seg_ctx.engine_info(0)
    assert rc == 0 and res[0]["status"] == 0 and info["engine"] == "segment-parallel", (key, info)
    assert np.array_equal(out, want) and (not filters or np.array_equal(f, wf)), key
    assert info["attempts"] + 1 == int(st[0]), (key, info, st)

"""GPU side of tests/test_seg_steps_host.py (-m gpu): the enumeration with compile-time step counts and the step's pre-based shared-memory operands
(pl_seg_core.h: seg_enum_body_k, seg_run_fast<F, TRX, N>, SegStepMem) through the library, the engine pinned to the segment engine, against the CPU
oracle bit for bit -- the same shapes (widths around one, two, three and nine segments, heights 4-6), every byte-per-pixel class, fully transparent
pixels, row_filters on and off, a state set of one chunk (s=19 b=2) and one of three (s=20 b=1); a batch of two images (blockIdx.y > 0); and the attempt
counts of the frames tests/test_seg_host.py pins, within its bounds: a wrong map or exit state costs attempts, never bytes."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu

WIDTHS = (1, 31, 32, 33, 65, 257)
HEIGHTS = (4, 5, 6)
MODES = (0, 2, 3, 4, 5)          # 4, 3, 2, 1 bytes per pixel; 5: four bytes with fully transparent pixels
PAIRS = ((19, 2), (20, 1))


@pytest.fixture()
def seg_ctx(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    ctx = P.HipContext()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("filters", [True, False], ids=["ids", "null"])
def test_single_images_match_oracle(seg_ctx, filters):
    for s, b in PAIRS:
        for w in WIDTHS:
            for h in HEIGHTS:
                for mode in MODES:
                    img = P.synth_rgba(w, h, mode, 0)
                    want, wf = U.run_port(img, s, b, filters=filters)
                    (out,), (f,), res = seg_ctx.run_host([img], s, b, want_filters=filters)
                    assert res[0]["status"] == 0 and seg_ctx.engine_info(0)["engine"] == "segment-parallel", (w, h, mode, s, b)
                    assert np.array_equal(out, want), (w, h, mode, s, b)
                    if filters:
                        assert np.array_equal(f, wf), (w, h, mode, s, b)


@pytest.mark.parametrize("s,b", PAIRS)
def test_a_batch_of_two_images_matches_oracle(seg_ctx, s, b):
    imgs = [P.synth_rgba(257, 6, 0, 0), P.synth_rgba(65, 5, 5, 0)]
    outs, filts, res = seg_ctx.run_host(imgs, s, b)
    for i, (img, out, f, r) in enumerate(zip(imgs, outs, filts, res)):
        want, wf = U.run_port(img, s, b)
        assert r["status"] == 0 and seg_ctx.engine_info(i)["engine"] == "segment-parallel"
        assert np.array_equal(out, want) and np.array_equal(f, wf), (i, s, b)


@pytest.mark.parametrize("h,s,b,most,most_restarts", [(128, 19, 2, 128 + 24, 12), (96, 20, 1, 130, None)])
def test_the_change_costs_no_attempts(seg_ctx, h, s, b, most, most_restarts):
    """the bounds of tests/test_seg_host.py for the same frames: test_seg_engine_speculation_is_right_almost_always (1024 x 128, s=19 b=2) and
    test_seg_engine_speculation_with_state_sets_enumerated_in_chunks (1024 x 96, s=20 b=1)"""
    img = P.synth_rgba(1024, h, 0, 0)
    want, wf = U.run_port(img, s, b)
    (out,), (f,), res = seg_ctx.run_host([img], s, b)
    info = seg_ctx.engine_info(0)
    assert res[0]["status"] == 0 and info["engine"] == "segment-parallel" and np.array_equal(out, want) and np.array_equal(f, wf)
    assert info["attempts"] <= most and info["serial_rows"] == 0, info
    if most_restarts is not None:
        assert info["restarts"] <= most_restarts, info

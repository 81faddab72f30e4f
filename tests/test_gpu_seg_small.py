"""GPU side of tests/test_seg_small_host.py (-m gpu): the table path of the enumeration body of none / up (pl_seg_core.h: seg_enum_small_body) on the device, the segment
engine pinned.  The smallest shapes at which the body can go wrong -- widths around one segment and around the four segments of a workgroup, heights 4 .. 6, every
byte-per-pixel class and fully transparent pixels -- at (19, 2) and (7, 1): bytes and filter IDs equal to the restatement's, and exactly the attempts the CPU harness
takes for the same input (the harness counts the attempt whose control launch finds the image finished, the device's record the one in front of it:
tests/test_gpu_seg_head.py).  And one image of the suite with few colours, where candidate none stays alive in most rows."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu

WIDTHS = (1, 31, 32, 33, 127, 128, 129, 257)
MODES = (0, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def seg_ctx():
    import os
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    before = os.environ.get("PNGLOSS_HIP_ENGINE")
    os.environ["PNGLOSS_HIP_ENGINE"] = "seg"
    ctx = P.HipContext()
    yield ctx
    ctx.close()
    if before is None:
        del os.environ["PNGLOSS_HIP_ENGINE"]
    else:
        os.environ["PNGLOSS_HIP_ENGINE"] = before


def check(seg_ctx, img, s, b, what):
    want, wf = U.run_port(img, s, b)
    rc, host_out, host_f, st = U.run_seg_host(img, s, b)
    assert rc == 0 and np.array_equal(host_out, want) and np.array_equal(host_f, wf), what
    (out,), (f,), res = seg_ctx.run_host([img], s, b)
    info = seg_ctx.engine_info(0)
    assert res[0]["status"] == 0 and info["engine"] == "segment-parallel", (what, info)
    assert np.array_equal(out, want) and np.array_equal(f, wf), what
    assert info["attempts"] + 1 == int(st[0]), (what, info, st)


@pytest.mark.parametrize("s,b", [(19, 2), (7, 1)])
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_and_classes_match_oracle_in_the_harness_attempts(seg_ctx, w, s, b):
    for k, mode in enumerate(MODES):
        h = 4 + (k + w) % 3
        check(seg_ctx, P.synth_rgba(w, h, mode, w + k), s, b, (w, h, mode, s, b))


def test_few_colours_keep_none_alive(seg_ctx):
    g = U.load_npz("suite_small.npz")
    img = np.ascontiguousarray(g["tux/in"])
    (out,), (f,), res = seg_ctx.run_host([img], 19, 2)
    info = seg_ctx.engine_info(0)
    assert res[0]["status"] == 0 and info["engine"] == "segment-parallel", info
    assert np.array_equal(out, g["tux/out"]) and np.array_equal(f, g["tux/filters"])
    rc, _, _, st = U.run_seg_host(img, 19, 2)
    assert rc == 0 and info["attempts"] + 1 == int(st[0]), (info, st)

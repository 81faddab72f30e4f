"""The enumeration launch on the device (-m gpu) behind tests/test_seg_enum_order_host.py: its candidates in the order the dispatch hands them out, the steps
behind the dedupe on one wave and on two, with the enumeration's workgroups pinned to 512 and to 1024 threads (PNGLOSS_HIP_ENUM_NT), the segment engine pinned.  Shapes: 256 x 6 (eight segments), 1056 x 3 (33 whole segments: a second replay
group of one segment) and 1050 x 3 (33 segments, the last one of 26 pixels); an exhaustive state set of one chunk (s=19 b=2: the distinct states fit one wave
nearly always) and one of several chunks (s=40 b=2: more than 64 states survive the dedupe, a second wave walks with the first).
Pixels and filter bytes equal the CPU oracle's (tests/util.py: run_port), the attempts are those of the CPU harness of the same bodies (run_seg_host, which
counts the control launch that finds the image finished: one more), and the library says which engine ran."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu

SHAPES = ((256, 6), (1056, 3), (1050, 3))
PAIRS = ((19, 2), (40, 2))

_reference = {}


def reference(w, h, s, b):
    """the oracle's result and the harness's attempts for a case, computed once and shared by both thread counts"""
    key = (w, h, s, b)
    if key not in _reference:
        img = P.synth_rgba(w, h, 0, w + h)
        want, wf = U.run_port(img, s, b)
        rc, host_out, host_f, st = U.run_seg_host(img, s, b)
        assert rc == 0 and np.array_equal(host_out, want) and np.array_equal(host_f, wf), key
        for a in (img, want, wf):
            a.setflags(write=False)
        _reference[key] = (img, want, wf, int(st[0]))
    return _reference[key]


@pytest.fixture(params=(512, 1024))
def seg_ctx(request, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("PNGLOSS_HIP_ENGINE", "seg")
    monkeypatch.setenv("PNGLOSS_HIP_ENUM_NT", str(request.param))
    ctx = P.HipContext()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("s,b", PAIRS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_tail_of_the_enumeration_matches_oracle_in_the_harness_attempts(seg_ctx, w, h, s, b):
    img, want, wf, host_attempts = reference(w, h, s, b)
    (out,), (f,), res = seg_ctx.run_host([img.copy()], s, b)
    info = seg_ctx.engine_info(0)
    assert res[0]["status"] == 0 and info["engine"] == "segment-parallel", (w, h, s, b, info)
    assert np.array_equal(out, want) and np.array_equal(f, wf), (w, h, s, b)
    assert info["attempts"] + 1 == host_attempts, (w, h, s, b, info, host_attempts)

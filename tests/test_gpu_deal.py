"""GPU test of the edges of the multi-GPU wrapper's deal (pl_deal.h, pl_host.hip: deal_over_contexts) that the two-context tests of the three forms leave
open: no image at all, one image (a context gets nothing), and an image without pixels dealt to a context next to widths off every alignment.  Two
contexts on one device must give, image by image, what one context gives.  Equality is exact."""
import numpy as np
import pytest

import pngloss_amd as P

pytestmark = pytest.mark.gpu

BLEED = 2
#: (width, height, synth mode).  The last batch: LPT puts 33 x 5 on context 0, 16 x 8 and the empty image on context 1.
BATCHES = {"none": [], "one": [(16, 8, 0)], "three": [(16, 8, 0), (0, 0, 0), (33, 5, 2)]}


@pytest.fixture(scope="module")
def pair():
    one, two = P.HipMulti("0"), P.HipMulti("0,0")
    try:
        assert (one.count, two.count) == (1, 2)
        for m in (one, two):
            m.set_option("distortion", "on")
        yield one, two
    finally:
        one.close()
        two.close()


def _same_images(a, b, n):
    """outs, filters, results of two calls"""
    assert len(a[0]) == len(b[0]) == n
    for i in range(n):
        assert np.array_equal(a[0][i], b[0][i]) and np.array_equal(a[1][i], b[1][i]) and a[2][i] == b[2][i], i


@pytest.mark.parametrize("name", list(BATCHES))
def test_two_contexts_give_what_one_gives_on_the_edges_of_the_deal(pair, name):
    one, two = pair
    shapes = BATCHES[name]
    imgs = [P.synth_rgba(w, h, mode) if w * h else np.zeros((h, w, 4), np.uint8) for (w, h, mode) in shapes]
    n = len(imgs)
    if name == "three":
        assert P.multi_split([(w, h) for (w, h, _) in shapes], 2) == [1, 1, 0]

    # the plain form leaves a last batch per context: the records are indexed through the deal
    a, b = one.run_host(imgs, 19, BLEED), two.run_host(imgs, 19, BLEED)
    _same_images(a, b, n)
    for i in range(n):
        assert two.distortion(i).as_dict() == one.distortion(i).as_dict(), i
        assert two.distortion(i).pixels == shapes[i][0] * shapes[i][1]
    for m in pair:
        with pytest.raises(RuntimeError):
            m.distortion(n)

    # the target form: its records are in the reports, and there is no last batch to index afterwards
    target = P.Target(38.0, 0, 19)
    a, b = one.run_host_target(imgs, target, BLEED, emit="scanlines"), two.run_host_target(imgs, target, BLEED, emit="scanlines")
    _same_images(a, b, n)
    for i in range(n):
        assert a[3][i].as_dict() == b[3][i].as_dict(), i
        assert a[4][i][0] == b[4][i][0] and np.array_equal(a[4][i][1], b[4][i][1]) and np.array_equal(a[4][i][2], b[4][i][2]), i
    for m in pair:
        with pytest.raises(RuntimeError):
            m.distortion(0)

    # the size form, budgets travelling with their images: the same
    budgets = [(w * 4 + 1) * h // 3 for (w, h, _) in shapes]
    a, b = one.run_host_size(imgs, budgets, 19, BLEED, emit="zlib"), two.run_host_size(imgs, budgets, 19, BLEED, emit="zlib")
    _same_images(a, b, n)
    for i in range(n):
        assert a[3][i].as_dict() == b[3][i].as_dict(), i
        assert a[5][i] == b[5][i], i
        if not shapes[i][0] * shapes[i][1]:
            assert (b[3][i].strength, b[3][i].probes, b[3][i].runs, b[3][i].reached, b[3][i].bytes) == (0, 0, 0, 1, 0)
    for m in pair:
        with pytest.raises(RuntimeError):
            m.distortion(0)

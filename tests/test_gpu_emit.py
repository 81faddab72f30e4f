"""The emit kernels (pngloss_amd/csrc/pl_emit.hip: pl_emit_classify, pl_emit_rows) through pngloss_hip_optimize_batch_host_emit, against the numpy
restatement of the reference's writer (tests.util.png_scanlines_reference, itself held to real libpng by tests/test_emit_reference_host.py) applied to
the ORACLE's output: colour type, filter type of every row and the filtered bytes, all exactly, in both row_filters modes, at strength 0 and 19.
Shapes where the kernels take another path: one-pixel-wide and one-pixel-high images (libpng drops the filters without a neighbour), a batch whose grid
is sized by its tallest image, rows beyond the 1024 pixels one pass of the filter-and-repack loop covers, and a single pixel that decides the class."""
import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U

pytestmark = pytest.mark.gpu

CLASSES = ("rgba", "rgb", "graya", "gray")
MODES = [(s, wf) for s in (0, 19) for wf in (True, False)]
MODE_IDS = ["s%d_%s" % (s, "ids" if wf else "null") for s, wf in MODES]


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext(0)
    yield c
    c.close()


def check_batch(ctx, imgs, strength, want_filters, names=None):
    """one emit call for the batch; every image against the restatement of the oracle's result.  Returns the colour types."""
    outs, filts, emitted = ctx.run_host_emit(imgs, strength, 2, want_filters=want_filters)
    types, wrong = [], []
    for i, (a, o, f, (ctype, ids, rows)) in enumerate(zip(imgs, outs, filts, emitted)):
        what = (names[i] if names else i, a.shape)
        o1, f1 = U.run_port(a, strength, 2, want_filters)
        assert np.array_equal(o, o1), what
        if want_filters:
            assert np.array_equal(f, f1), what
        want_ct, want_ids, want_rows = U.png_scanlines_reference(o1, f1 if want_filters else None)
        if ctype != want_ct:
            wrong.append((what, "colour type", ctype, want_ct))
        elif not np.array_equal(ids, want_ids):
            y = int(np.flatnonzero(ids != want_ids)[0])
            wrong.append((what, "filter type of row %d" % y, int(ids[y]), int(want_ids[y])))
        elif not np.array_equal(rows, want_rows):
            wrong.append((what, "filtered bytes"))
        types.append(ctype)
    # (every image that differs, not only the first)
    assert not wrong, "strength %d, want_filters %s: %d of %d images differ\n" % (strength, want_filters, len(wrong), len(imgs)) + "\n".join(map(str, wrong))
    return types


@pytest.mark.parametrize("strength,want_filters", MODES, ids=MODE_IDS)
def test_one_pixel_wide_and_one_pixel_high_images(ctx, strength, want_filters):
    """every image of tests/golden/emit_degenerate.npz: widths and heights 1, 2, 40 and 700 in every class, and one-row images on which "average" has the
    smallest sum.  At strength 0 the pixels are the recorded ones, so what libpng itself chose for them is compared too."""
    fixture = U.emit_degenerate_fixture()
    imgs = [rgba for _, rgba, _, _ in fixture]
    check_batch(ctx, imgs, strength, want_filters, names=[name for name, _, _, _ in fixture])
    if strength == 0 and not want_filters:
        _, _, emitted = ctx.run_host_emit(imgs, 0, 2, want_filters=False)
        for (name, _, ctype, lines), (got_ct, ids, rows) in zip(fixture, emitted):
            assert got_ct == ctype, name
            assert np.array_equal(np.concatenate([ids[:, None], rows], axis=1), lines[U.EMIT_POLICIES.index(-1)]), name


@pytest.mark.parametrize("strength,want_filters", MODES, ids=MODE_IDS)
def test_batch_of_mixed_heights(ctx, strength, want_filters):
    """heights 1, 2, 40 and 700 in one batch: the grid has 700 rows of workgroups for every image, those past an image's height exit early"""
    rng = np.random.default_rng(31)
    shapes = [(50, 1), (1, 700), (3, 2), (33, 40), (5, 700), (1, 2), (300, 1), (64, 40), (1, 1), (7, 2)]
    imgs = [U.as_pixel_class(rng.integers(0, 256, (h, w, 4), dtype=np.uint8) // 8 * 8, CLASSES[i % 4]) for i, (w, h) in enumerate(shapes)]
    check_batch(ctx, imgs, strength, want_filters)


@pytest.mark.parametrize("strength,want_filters", MODES, ids=MODE_IDS)
def test_rows_around_and_beyond_one_pass_of_the_repack_loop(ctx, strength, want_filters):
    """256 lanes take four pixels each: 1024 pixels a pass.  1023 and 1025 leave a ragged quad, 4099 = four passes and three pixels."""
    rng = np.random.default_rng(32)
    imgs = [U.as_pixel_class(rng.integers(0, 256, (3, w, 4), dtype=np.uint8), cls) for w in (1023, 1024, 1025, 4099) for cls in CLASSES]
    types = check_batch(ctx, imgs, strength, want_filters)
    if strength == 0:
        assert types == [6, 2, 4, 0] * 4


# 130 x 70 = 9100 pixels: three classify workgroups of 256 lanes that stride over the image together; pixel i belongs to workgroup (i // 256) % 3
ODD_PIXELS = {"first": (0, 0), "middle_workgroup": (32, 40), "last": (69, 129)}


@pytest.mark.parametrize("want_filters", [True, False], ids=["ids", "null"])
def test_one_pixel_decides_the_colour_type(ctx, want_filters):
    rng = np.random.default_rng(33)
    base = U.as_pixel_class(rng.integers(0, 256, (70, 130, 4), dtype=np.uint8), "gray")
    assert [((y * 130 + x) // 256) % 3 for (y, x) in ODD_PIXELS.values()] == [0, 1, 2]
    imgs, want = [base], [0]
    for (y, x) in ODD_PIXELS.values():
        for kind, ctype in (("coloured", 2), ("alpha", 4), ("both", 6)):
            a = base.copy()
            if kind in ("coloured", "both"):
                a[y, x, 0] ^= 1
            if kind in ("alpha", "both"):
                a[y, x, 3] = 254
            imgs.append(a); want.append(ctype)
    # the coloured pixel and the translucent one in different workgroups
    a = base.copy(); a[0, 0, 2] ^= 128; a[69, 129, 3] = 254
    imgs.append(a); want.append(6)
    assert check_batch(ctx, imgs, 0, want_filters) == want

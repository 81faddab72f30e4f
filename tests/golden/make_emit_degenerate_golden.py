"""Record what the REAL reference's writer (libpng, through oracle/_ref/rwpng_copy_ref) hands zlib for one-pixel-wide and one-pixel-high images, where
libpng drops the filters that have no neighbour to predict from, so that tests/test_emit_reference_host.py can hold the numpy restatement of the write
side (tests.util.png_scanlines_reference) to it where oracle/_ref is not built, and tests/test_gpu_emit.py has the images.

Run where oracle/_ref is built (`make -C oracle`):   python tests/golden/make_emit_degenerate_golden.py

Output (data only -- inputs and what the binary wrote for them):
  tests/golden/emit_degenerate.npz   per image  "<name>/rgba"   the input pixels (H, W, 4)
                                                "<name>/ctype"  the colour type of the file written
                                                "<name>/lines"  (7, H, 1 + W * channels): for the policies -1, 0..5 of tests/c/rwpng_copy.c
                                                                (tests.util.EMIT_POLICIES) the filter-type byte and the filtered bytes of every scanline
Images: the sizes SIZES in the four byte-per-pixel classes (RGBA, RGB, gray + alpha, gray), and one-row images on which the plain five-filter
minimum-sum heuristic would pick "average" (asserted here), which libpng does not allow in a one-row image."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import util as U  # noqa: E402

SIZES = [(1, 1), (2, 1), (1, 2), (40, 1), (1, 40), (2, 40), (40, 2), (700, 1), (1, 700)]
CLASSES = ["rgba", "rgb", "graya", "gray"]
CTYPE = dict(rgba=6, rgb=2, graya=4, gray=0)
#: seeds of average_wins_candidate whose RGBA image has the strictly smallest sum under "average"
AVERAGE_WINS_RGBA_SEEDS = (2, 7, 8)


def average_wins_candidate(seed, cls):
    rng = np.random.default_rng(seed)
    w = int(rng.integers(2, 60))
    return U.as_pixel_class(rng.integers(0, 256, (1, w, 4), dtype=np.uint8), cls)


def plain_argmin_one_row(img, cls):
    """the filter the minimum-sum heuristic picks among ALL five for a one-row image (the row above counts as zeros): the first of the smallest sums"""
    raw = {"rgba": img, "rgb": img[..., :3], "graya": img[..., [1, 3]], "gray": img[..., 1:2]}[cls]
    ch = raw.shape[2]
    cur = raw.reshape(-1).astype(np.int32)
    left = np.concatenate([np.zeros(ch, np.int32), cur[:-ch]])
    # no row above: up predicts 0, average half of the left neighbour, paeth the left neighbour
    sums = [int(np.where(r < 128, r, 256 - r).sum()) for r in [(cur - q) & 255 for q in (0 * cur, left, 0 * cur, left >> 1, left)]]
    return sums.index(min(sums)), sums


def images():
    out = []
    rng = np.random.default_rng(20261019)
    for (w, h) in SIZES:
        for cls in CLASSES:
            img = U.as_pixel_class(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), cls)
            if cls in ("rgba", "graya"):
                img[0, 0, 3] = 128                     # (a one-pixel image must not be opaque by chance)
            if cls in ("rgba", "rgb"):
                img[0, 0, :3] = (10, 20, 30)           # (nor gray)
            out.append(("%s_%dx%d" % (cls, w, h), cls, img))
    for seed in AVERAGE_WINS_RGBA_SEEDS:
        out.append(("rgba_average_wins_seed%d" % seed, "rgba", average_wins_candidate(seed, "rgba")))
    for cls in CLASSES:
        found = 0
        for seed in range(1000):
            if cls == "rgba" and seed in AVERAGE_WINS_RGBA_SEEDS:
                continue
            img = average_wins_candidate(seed, cls)
            best, sums = plain_argmin_one_row(img, cls)
            if best == 3 and sums[3] < min(sums[0], sums[1]):
                out.append(("%s_average_wins_seed%d" % (cls, seed), cls, img))
                found += 1
                if found == 2:
                    break
        assert found == 2, cls
    return out


def main():
    assert os.path.exists(U.REF_RWPNG), "build oracle/_ref first: make -C oracle"
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, cls, img in images():
            if "average_wins" in name:
                best, sums = plain_argmin_one_row(img, cls)
                assert best == 3 and sums[3] < min(sums[0], sums[1], sums[2], sums[4]), (name, sums)
            lines = []
            for policy in U.EMIT_POLICIES:
                ctype, got = U.ref_writer_scanlines(img, policy, tmp)
                assert ctype == CTYPE[cls], (name, policy, ctype)
                lines.append(got)
            arrays[name + "/rgba"] = img
            arrays[name + "/ctype"] = np.int32(CTYPE[cls])
            arrays[name + "/lines"] = np.stack(lines)
    path = os.path.join(HERE, "emit_degenerate.npz")
    np.savez_compressed(path, **arrays)
    print(len(arrays) // 3, "images,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""The keep arena of the distortion measurement (pl_keep_layout, pngloss_amd/csrc/pl_layout.h) on the CPU through tests/c/keep_layout_host.cpp:
what a GPU run would only show as a corrupted neighbour -- every region on a 256-byte boundary, no two overlapping, the total covering the last --
and the offsets themselves, restated here in Python."""
import numpy as np

from tests import util_distort as D
from tests.test_layout_host import A, au, check_regions

JOB, REC = 32, 64


def py_keep(ws, hs, originals, job=JOB, rec=REC):
    n = len(ws)
    o = 0
    jobs = o; o = au(o + job * (n or 1))
    records = o; o = au(o + rec * (n or 1))
    image = []
    for w, h in zip(ws, hs):
        if originals:
            image.append(o); o = au(o + w * h * 4)
        else:
            image.append(0)
    return image, dict(jobs=jobs, records=records, total=o)


def regions(ws, hs, image, t, originals):
    n = len(ws)
    r = [("jobs", t["jobs"], JOB * (n or 1)), ("records", t["records"], REC * (n or 1))]
    if originals:
        r += [("image%d" % i, image[i], ws[i] * hs[i] * 4) for i in range(n)]
    return r


def test_keep_arena_is_aligned_disjoint_and_pinned():
    rng = np.random.default_rng(9)
    for trial in range(300):
        n = int(rng.integers(0, 40))
        ws = [int(rng.choice([0, 1, 3, 63, 64, 65, 257, 1024, int(rng.integers(1, 5000))])) for _ in range(n)]
        hs = [int(rng.choice([0, 1, 3, 5, 7, int(rng.integers(1, 3000))])) for _ in range(n)]
        for originals in (True, False):
            image, t = D.keep_layout(ws, hs, originals)
            assert (image, t) == py_keep(ws, hs, originals), (ws, hs, originals)
            check_regions(regions(ws, hs, image, t, originals), t["total"], (ws, hs, originals))


def test_keep_arena_edge_cases():
    # n = 0: the two tables still have room for one entry each, and nothing else
    image, t = D.keep_layout([], [], True)
    assert image == [] and t == dict(jobs=0, records=A, total=2 * A)
    # images without pixels take no room but have an (aligned) place; their neighbours do not move onto each other
    # (five jobs: 160 bytes, one unit; five records: 320 bytes, two units; 7 x 3 and 3 x 1 pixels: one unit each)
    image, t = D.keep_layout([0, 5, 7, 0, 3], [9, 0, 3, 0, 1], True)
    assert t["jobs"] == 0 and t["records"] == A and image == [3 * A, 3 * A, 3 * A, 4 * A, 4 * A] and t["total"] == 5 * A
    # the tables grow with the batch: 9 jobs of 32 bytes are two 256-byte units, 9 records of 64 bytes are three
    image, t = D.keep_layout([1] * 9, [1] * 9, False)
    assert t == dict(jobs=0, records=2 * A, total=2 * A + au(9 * REC)) and image == [0] * 9
    # a 4096 x 4096 frame: 64 MiB behind the tables; beyond 2^32 bytes the offsets stay exact
    image, t = D.keep_layout([4096], [4096], True)
    assert image == [2 * A] and t["total"] == 2 * A + (64 << 20)
    image, t = D.keep_layout([40000, 40000], [30000, 1], True)
    assert image[1] == 2 * A + au(40000 * 30000 * 4) and t["total"] == image[1] + au(160000)

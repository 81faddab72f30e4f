"""CPU tests of the rules of the kernels around the row engine (pngloss_amd/csrc/pl_prepost_core.h, shared with pl_prepost.hip; no GPU): pl_hist's
thread loop run on the CPU under the sanitizers in the kernel's order -- both loaders, several workgroups, several trips -- against the oracle's
port_orig_histograms and a numpy restatement; the byte-wise arithmetic over every byte pair; the loader predicate, the loaders' index arithmetic, the
rank rule and the launch shapes against Python restatements (tests/util_prepost.py).  Expected values never come from the code under test."""
import numpy as np
import pytest

from tests import util_prepost as R


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_prepost_host(tmp_path_factory.mktemp("prepost_host"))


def test_tables_equal_the_oracle_and_numpy_under_asan_and_ubsan(exe, tmp_path):
    """every shape of the GPU tests in the launch shape the device gives it (two workgroups of 1024), and small ones in odd launch shapes: one lane,
    more lanes than steps, a stride that is no multiple of the row, bases 4 and 8 bytes off 16 (the quad loader must then not run)"""
    cases, want = [], []

    def add(w, h, kind, cls, off, blocks, threads):
        bpp = R.BPP_OF_CLASS[cls]
        img = R.content(w, h, kind, cls)
        cases.append((R.slots(img, bpp), bpp, off, blocks, threads))
        want.append((w, h, kind, cls, off))

    for w, h, loader in R.SHAPES:
        blocks, trips = R.hist_trips(1, w * h, w, h)
        assert blocks == 2 and trips >= 2 and R.quad_loader(w, 0, w * h) == (loader == "quad")
        for k, cls in enumerate(R.CLASSES):
            add(w, h, ("noise", "four")[k % 2], cls, 0, blocks, 1024)
    for off in (4, 8):
        assert R.hist_trips(1, 164 * 101, 164, 101, aligned=False) == (2, 9)
        add(164, 101, "noise", "rgba", off, 2, 1024)
    add(164, 101, "flat", "rgb", 0, 2, 1024)
    for w, h in ((1, 1), (4, 1), (5, 1), (1, 5), (4, 3), (8, 5), (12, 7), (13, 7), (64, 2)):
        for blocks, threads in ((1, 1), (3, 5), (2, 64), (7, 3)):
            add(w, h, "noise", R.CLASSES[(w + h + blocks) % 4], 0, blocks, threads)
            add(w, h, "four", R.CLASSES[(w + blocks) % 4], 4, blocks, threads)
    got = R.run_cases(exe, tmp_path, cases)
    for (w, h, kind, cls, off), (img, bpp, _, blocks, threads), (freq, rank, quad, pixels) in zip(want, cases, got):
        what = (w, h, kind, cls, off, blocks, threads)
        pk = R.packed(R.content(w, h, kind, cls), bpp)
        assert quad == R.quad_loader(w, off, w * h) and pixels == w * h, what
        assert np.array_equal(freq, R.oracle_orig_tables(pk)), what
        assert np.array_equal(freq, R.np_orig_tables(pk)), what
        assert (freq.sum(axis=1) == bpp * w * h).all(), what
        assert np.array_equal(rank, R.rank_rule(freq)), what
    # the flat image: a handful of bins hold everything -- per channel the value, 0, and under "average" the value less its half along two edges
    flat = got[len(R.SHAPES) * 4 + 2][0]
    assert np.count_nonzero(flat, axis=1).tolist() == [3, 4, 4, 7, 4] and flat[0].max() == 164 * 101


def test_sub4_and_avg4_over_every_byte_pair_in_every_lane(exe, tmp_path):
    out = str(tmp_path / "bytes.bin")
    assert R.run_host(exe, ["bytes", out]) == []
    got = np.fromfile(out, np.uint32).reshape(4, 2, 2, 256, 256, 2)
    a, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for lane in range(4):
        for fa in (0, 1):
            for fb in (0, 1):
                oa, ob = 255 * fa, 255 * fb
                # the other three lanes hold (oa, ob): their results must be those of that pair, whatever this lane does -- no carry, no borrow
                want_sub = sum((((a if k == lane else oa) - (b if k == lane else ob)) & 255) << (8 * k) for k in range(4))
                want_avg = sum((((a if k == lane else oa) + (b if k == lane else ob)) >> 1) << (8 * k) for k in range(4))
                assert np.array_equal(got[lane, fa, fb, :, :, 0], want_sub.astype(np.uint32)), (lane, fa, fb)
                assert np.array_equal(got[lane, fa, fb, :, :, 1], want_avg.astype(np.uint32)), (lane, fa, fb)


def test_loader_predicate_at_its_three_edges(exe):
    base = 1 << 20
    points = [(164, base, 164 * 101), (163, base, 163 * 101), (162, base, 162 * 2), (4, base, 16), (8, base + 16, 64), (0, base, 0)]          # W % 4
    points += [(164, base + off, 164 * 101) for off in (4, 8, 12, 16, 1, 15)]                                                                 # the pointer
    points += [(4, base, 0xFFFFFFFE), (4, base, 0xFFFFFFFF), (4, base, 1 << 32), (65536, base, 65536 * 65535), (65536, base, 65536 * 65536)]   # n < 2^32 - 1
    got = [int(x) for x in R.run_host(exe, ["loader"] + [v for p in points for v in p])]
    assert got == [int(R.quad_loader(*p)) for p in points]
    assert got == [1, 0, 0, 1, 1, 1] + [0, 0, 0, 1, 0, 0] + [1, 0, 0, 1, 0]


def test_loaders_index_arithmetic(exe):
    quads = [(q, w4) for w4 in (1, 2, 41, 1366) for q in (0, 1, w4 - 1, w4, w4 + 1, 2 * w4 - 1, 2 * w4, 5 * w4 + w4 // 2)] + [(0x3FFFFFFE, 41), (0xFFFFFFFD, 0x7FFFFFFF)]
    got = [[int(x) for x in line.split()] for line in R.run_host(exe, ["quad"] + [v for p in quads for v in p])]
    for (q, w4), g in zip(quads, got):
        up, left = q >= w4, q % w4 != 0
        assert g == [int(up), int(left), q - w4 if up else 0, 4 * q - 1 if left else 0, 4 * (q - w4) - 1 if up and left else 0], (q, w4)
    pixels = [(i, w) for w in (1, 2, 163, 5465) for i in (0, 1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 7 * w + w // 2)] + [((1 << 33) + 5, 163), ((1 << 33), 1 << 31)]
    got = [[int(x) for x in line.split()] for line in R.run_host(exe, ["pixel"] + [v for p in pixels for v in p])]
    for (i, w), g in zip(pixels, got):
        up, left = i >= w, i % w != 0
        assert g == [int(up), int(left), i - w if up else 0, i - 1 if left else 0, i - w - 1 if up and left else 0], (i, w)


def test_rank_on_equal_distinct_and_tied_counts(exe, tmp_path):
    rng = np.random.default_rng(7)
    equal = np.full(256, 12345, np.uint32)
    zeros = np.zeros(256, np.uint32)
    distinct = rng.permutation(256).astype(np.uint32) * 3 + 1
    ties = np.array([0, 0, 7, 7, 7, 9, 0, 2 ** 32 - 1] * 32, np.uint32)           # ties with zeros, and the largest count a bin can hold
    few = zeros.copy()
    few[[3, 200]] = (5, 5)
    tables = [equal, zeros, distinct, ties, few]
    path = str(tmp_path / "rank.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([len(tables)], np.uint64).tobytes())
        for t in tables:
            fh.write(t.tobytes())
    got = [np.array(line.split(), np.int64) for line in R.run_host(exe, ["rank", path])]
    for t, g in zip(tables, got):
        assert np.array_equal(g, R.rank_rule(t[None])[0])
    assert not got[0].any() and not got[1].any()
    assert np.array_equal(got[2], (distinct - 1) // 3) and sorted(got[2]) == list(range(256))
    assert sorted(set(got[3])) == [0, 96, 192, 224] and got[4][3] == got[4][200] == 254 and got[4].sum() == 2 * 254
    # order and equality are kept: a < b <=> rank(a) < rank(b), a == b <=> rank(a) == rank(b)
    for t, g in zip(tables, got):
        t = t.astype(np.int64)
        assert np.array_equal(np.sign(t[:, None] - t[None, :]), np.sign(g[:, None] - g[None, :]))


def test_grid_rules_equal_their_restatement_at_the_pinned_points(exe):
    assert R.GRID_N == [1, 5, 191, 192, 256, 257, 2048, 65535]
    items, want = [], []
    for max_px in sorted(R.GRID_HIST):
        for n in R.GRID_N:
            for shape in (R.HIST_DEFAULT, R.HIST_VARIANT):
                items += ["hist", n, max_px, shape[0], shape[1]]
                want.append(R.hist_blocks(n, max_px, shape))
    for max_px in sorted(R.GRID_BATCH16) + [2048, 2049, 84000]:
        for n in R.GRID_N:
            for ppt in (16, 8):
                items += ["batch", n, max_px, ppt]
                want.append(R.batch_blocks(n, max_px, ppt))
    slices = [(1, 0), (65535, 0), (65536, 0), (65536, 65535), (65540, 0), (65540, 65535), (200000, 131070), (200000, 196605)]
    for n, first in slices:
        items += ["slice", n, first]
        want.append(R.slice_images(n, first))
    lines = R.run_host(exe, ["grid"] + items)
    assert lines[0].split() == ["65535", "256"] and (R.MAX_IMAGES, R.THREADS) == (65535, 256)
    got = [int(x) for x in lines[1:]]
    assert got == want
    # the restatement itself, at written-out values
    for max_px, blocks in R.GRID_HIST.items():
        assert [R.hist_blocks(n, max_px) for n in R.GRID_N] == blocks, max_px
    for max_px, blocks in R.GRID_BATCH16.items():
        assert [R.batch_blocks(n, max_px, 16) for n in R.GRID_N] == blocks, max_px
    assert want[-len(slices):] == [1, 65535, 65535, 1, 65535, 5, 65535, 3395]
    # what the GPU tests rely on
    assert R.hist_blocks(1, 164 * 101, R.HIST_VARIANT) == 5 and R.hist_blocks(200, 300 * 280) == 4 < R.hist_blocks(1, 300 * 280) == 6

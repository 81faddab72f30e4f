"""GPU tests of the kernels that every optimise call runs around the row engine (pl_prepost.hip, pl_rows.hip, pl_emit.hip, the deflate's launches):

* the tables pl_hist and pl_rank leave -- original_frequency and its 8-bit ranks, read back with pngloss_hip_last_original_tables -- on the
  smallest shapes that give pl_hist a second workgroup and a lane a second trip, through both loaders, in the four byte-per-pixel classes, under a
  capped grid, in the second variant of the kernel, and the table the strength-0 engine sums from its rows' counts;
* batches of 65 540 images: every launch that has the batch in gridDim.y goes in slices of 65 535.

Everything by equality.  Pixels, filters and the final histogram come from the CPU oracle (U.run_port_packed), the tables from the oracle's
port_orig_histograms on the packed class and from the rank rule applied to them (tests/util_prepost.py); tests/test_prepost_host.py holds those
against a numpy restatement and the launch shapes against pl_prepost_core.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_prepost as R

pytestmark = pytest.mark.gpu

WG, ROWS = "workgroup-per-image", "row-statistics (strength 0)"


def _run_one(ctx, img, s=19, b=2, filters=True, offset=0):
    """one image from a device buffer that starts `offset` bytes behind a 16-byte boundary: (pixels, filters, result)"""
    import torch
    h, w = img.shape[:2]
    buf = torch.zeros(img.size + 32, dtype=torch.uint8, device="cuda")
    flt = torch.zeros(max(h, 1), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset: offset + img.size]
    view.copy_(torch.from_numpy(np.array(img).reshape(-1)))
    torch.cuda.synchronize()
    res = ctx.run([(view.data_ptr() if img.size else 0, flt.data_ptr() if filters else 0, w, h)], s, b)
    torch.cuda.synchronize()
    return view.cpu().numpy().reshape(h, w, 4), flt.cpu().numpy()[:h], res[0]


def _check_one(ctx, w, h, kind, cls, offset=0):
    """content(w, h, kind, cls) at (19, 2): pixels, filters, final histogram, both tables and their sums"""
    what = (w, h, kind, cls, offset)
    bpp = R.BPP_OF_CLASS[cls]
    want_out, want_f, want_hist, want_freq, want_rank = R.expected(w, h, kind, cls)
    out, f, res = _run_one(ctx, R.content(w, h, kind, cls), offset=offset)
    assert (res["status"], res["bpp"]) == (0, bpp) and ctx.engine_info(0)["engine"] == WG, what
    assert np.array_equal(out, want_out) and np.array_equal(f, want_f), what
    assert np.array_equal(ctx.histogram(0), want_hist), what
    freq, rank = ctx.original_tables(0)
    assert np.array_equal(freq, want_freq), (what, np.argwhere(freq != want_freq)[:8].tolist())
    assert np.array_equal(rank, want_rank), (what, np.argwhere(rank != want_rank)[:8].tolist())
    assert (freq.sum(axis=1, dtype=np.int64) == bpp * w * h).all(), what
    return freq, rank


@pytest.fixture()
def wg_ctx():
    ctx = P.HipContext()
    ctx.set_option("engine", "wg")
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ the tables, past one workgroup and one trip

@pytest.mark.parametrize("w,h,loader", R.SHAPES)
def test_tables_past_one_workgroup_and_one_trip(wg_ctx, w, h, loader):
    blocks, trips = R.hist_trips(1, w * h, w, h)
    assert blocks == 2 and trips >= 2 and R.quad_loader(w, 0, w * h) == (loader == "quad")        # the shape does cross both boundaries
    assert 16384 < w * h < 16384 + 512                                                              # ... and only just
    for cls in R.CLASSES:
        for kind in ("noise", "four") + (("flat",) if (w, h) == (164, 101) else ()):
            freq, rank = _check_one(wg_ctx, w, h, kind, cls)
            if kind == "four":
                assert (freq == 0).sum() > 1000 and len(np.unique(rank[0])) <= 5                   # zero and tied counts: equal ranks
            if kind == "flat":
                assert freq[0].max() * np.count_nonzero(freq[0]) == R.BPP_OF_CLASS[cls] * w * h    # every lane's atomics land on a few words


@pytest.mark.parametrize("offset", [4, 8])
def test_tables_from_a_pointer_off_16_bytes_take_the_scalar_loader(wg_ctx, offset):
    w, h = 164, 101
    assert R.quad_loader(w, 0, w * h) and not R.quad_loader(w, offset, w * h)
    assert R.hist_trips(1, w * h, w, h, aligned=False) == (2, 9) and R.hist_trips(1, w * h, w, h) == (2, 3)
    for cls in R.CLASSES:
        for kind in ("noise", "four"):
            _check_one(wg_ctx, w, h, kind, cls, offset=offset)


@pytest.mark.parametrize("w,h", [(0, 0), (0, 5)])
def test_tables_of_an_image_without_pixels_are_zero(wg_ctx, w, h):
    out, f, res = _run_one(wg_ctx, np.zeros((h, w, 4), np.uint8))
    assert res["status"] == 0 and out.size == 0
    freq, rank = wg_ctx.original_tables(0)
    assert not freq.any() and not rank.any()
    assert not wg_ctx.histogram(0).any()


def test_tables_under_a_capped_grid():
    """200 images in a call: pl_hist gets max(4, ceil(768 / 200)) = 4 workgroups per image where the two large ones want six, so their lanes go
    round more often than alone; the tables are those of the same images run alone, and the oracle's"""
    import torch
    big = [(300, 280, "noise", "rgba"), (299, 281, "noise", "rgb")]
    small = [(w, h, kind, cls) for (w, h) in ((13, 7), (8, 5), (64, 2), (12, 7), (1, 5)) for kind, cls in (("noise", "rgba"), ("four", "rgb"), ("noise", "graya"), ("four", "gray"))]
    specs = big + [small[i % len(small)] for i in range(198)]
    n = len(specs)
    max_px = 299 * 281
    assert n == 200 and R.hist_blocks(n, max_px) == 4 < R.hist_blocks(1, 300 * 280) == R.hist_blocks(1, max_px) == 6
    assert R.hist_trips(n, max_px, 300, 280) == (4, 6) and R.hist_trips(n, max_px, 299, 281) == (4, 21) and R.quad_loader(300, 0, 1)
    imgs = [R.content(*s) for s in specs]
    dev = [torch.from_numpy(np.array(a)).cuda() for a in imgs]
    flt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in imgs]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    look = [0, 1] + list(range(2, 198, 17))
    assert len(look) == 14
    ctx = P.HipContext()
    try:
        ctx.set_option("engine", "wg")
        res = ctx.run([(d.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for d, f, a in zip(dev, flt, imgs)], 19, 2)
        torch.cuda.synchronize()
        tables = {i: ctx.original_tables(i) for i in look}
        hists = {i: ctx.histogram(i) for i in look}
        for i in look:
            w, h, kind, cls = specs[i]
            want_out, want_f, want_hist, want_freq, want_rank = R.expected(*specs[i])
            assert res[i]["status"] == 0 and np.array_equal(dev[i].cpu().numpy(), want_out) and np.array_equal(flt[i].cpu().numpy(), want_f), (i, specs[i])
            alone_out, alone_f, _ = _run_one(ctx, imgs[i])
            alone = ctx.original_tables(0)
            assert np.array_equal(alone_out, want_out) and np.array_equal(alone_f, want_f), (i, specs[i])
            for got in (tables[i], alone):
                assert np.array_equal(got[0], want_freq) and np.array_equal(got[1], want_rank), (i, specs[i])
            assert np.array_equal(hists[i], want_hist), (i, specs[i])
    finally:
        ctx.close()


def test_tables_of_the_second_variant_of_the_kernel():
    """PNGLOSS_HIP_HIST=1 is read once per process: a fresh child runs 164 x 101 and 163 x 101 in the four classes on five workgroups of 256 threads
    and eight replicas (host form: the window's arena starts on 16 bytes), against the oracle's tables"""
    assert R.hist_blocks(1, 164 * 101, R.HIST_VARIANT) == R.hist_blocks(1, 163 * 101, R.HIST_VARIANT) == 5
    assert R.hist_trips(1, 164 * 101, 164, 101, shape=R.HIST_VARIANT) == (5, 4) and R.hist_trips(1, 163 * 101, 163, 101, shape=R.HIST_VARIANT) == (5, 13)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "import pngloss_amd as P\n"
            "from tests import util_prepost as R\n"
            "ctx = P.HipContext()\n"
            "ctx.set_option('engine', 'wg')\n"
            "for w in (164, 163):\n"
            "    for k, cls in enumerate(R.CLASSES):\n"
            "        kind = ('noise', 'four')[k %% 2]\n"
            "        want_out, want_f, want_hist, want_freq, want_rank = R.expected(w, 101, kind, cls)\n"
            "        outs, filts, res = ctx.run_host([R.content(w, 101, kind, cls)], 19, 2)\n"
            "        freq, rank = ctx.original_tables(0)\n"
            "        assert res[0]['status'] == 0 and np.array_equal(outs[0], want_out) and np.array_equal(filts[0], want_f), (w, cls)\n"
            "        assert np.array_equal(freq, want_freq) and np.array_equal(rank, want_rank) and np.array_equal(ctx.histogram(0), want_hist), (w, cls)\n"
            "ctx.close()\n"
            "print('variant ok')\n" % U.ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PNGLOSS_HIP_HIST="1"), timeout=300)
    assert r.returncode == 0 and "variant ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


@pytest.mark.parametrize("w,h,filters", [(164, 101, True), (164, 101, False), (163, 101, True), (5465, 3, True)])
def test_strength_0_sums_the_table_from_its_rows_counts(w, h, filters):
    """nothing pinned: strength 0 goes to the row-statistics engine, whose pl_rows_decide adds up the rows' counts of all five filters -- the four a
    row did not choose included.  It runs no pl_rank: asking for the ranks is refused."""
    lib = P.hip_lib()
    ctx = P.HipContext()
    try:
        for cls in R.CLASSES:
            what = (w, h, cls, filters)
            bpp = R.BPP_OF_CLASS[cls]
            img = R.content(w, h, "noise" if cls in ("rgba", "graya") else "four", cls)
            want_out, want_f, want_hist, want_freq, _ = R.expected(w, h, "noise" if cls in ("rgba", "graya") else "four", cls, 0, 2, filters)
            out, f, res = _run_one(ctx, img, 0, 2, filters)
            assert (res["status"], res["bpp"]) == (0, bpp) and ctx.engine_info(0)["engine"] == ROWS, what
            assert np.array_equal(out, want_out) and np.array_equal(out, img) and (not filters or np.array_equal(f, want_f)), what
            assert np.array_equal(ctx.histogram(0), want_hist), what
            freq, rank = ctx.original_tables(0)
            assert rank is None and np.array_equal(freq, want_freq), (what, np.argwhere(freq != want_freq)[:8].tolist())
            assert (freq.sum(axis=1, dtype=np.int64) == bpp * w * h).all(), what
            table = np.zeros((5, 256), np.uint32)
            assert lib.pngloss_hip_last_original_tables(ctx._ctx, 0, None, table.ctypes.data) == L.PNGLOSS_INVALID_ARGUMENT
            assert lib.pngloss_hip_last_original_tables(ctx._ctx, 0, table.ctypes.data, table.ctypes.data) == L.PNGLOSS_INVALID_ARGUMENT
            assert lib.pngloss_hip_last_original_tables(ctx._ctx, 0, table.ctypes.data, None) == 0 and np.array_equal(table, want_freq)
    finally:
        ctx.close()


def test_refusals_of_the_read_back():
    import torch
    lib = P.hip_lib()
    img = R.content(13, 7, "noise", "rgba")
    want_freq, want_rank = R.expected(13, 7, "noise", "rgba")[3:]
    freq, rank = np.zeros((5, 256), np.uint32), np.zeros((5, 256), np.uint32)
    call = lambda ctx, i, a, b: lib.pngloss_hip_last_original_tables(ctx._ctx, i, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None)
    ctx = P.HipContext()
    try:
        assert call(ctx, 0, freq, rank) == L.PNGLOSS_INVALID_ARGUMENT                               # no batch yet
        assert lib.pngloss_hip_last_original_tables(None, 0, freq.ctypes.data, rank.ctypes.data) == L.PNGLOSS_INVALID_ARGUMENT
        d, f = torch.from_numpy(np.array(img)).cuda(), torch.zeros(7, dtype=torch.uint8, device="cuda")
        desc = [(d.data_ptr(), f.data_ptr(), 13, 7)]
        ctx.enqueue(desc, 19, 2)
        assert call(ctx, 0, freq, rank) == L.PNGLOSS_INVALID_ARGUMENT                               # a batch in flight
        ctx.finish()
        assert call(ctx, 0, None, None) == L.PNGLOSS_INVALID_ARGUMENT                               # both NULL
        assert call(ctx, 1, freq, rank) == L.PNGLOSS_INVALID_ARGUMENT                               # out of range
        assert call(ctx, 2 ** 63, freq, rank) == L.PNGLOSS_INVALID_ARGUMENT
        assert not freq.any() and not rank.any()                                                    # a refused call writes nothing
        assert call(ctx, 0, freq, None) == 0 and np.array_equal(freq, want_freq) and not rank.any()
        assert call(ctx, 0, None, rank) == 0 and np.array_equal(rank, want_rank)
        d.copy_(torch.from_numpy(np.array(img)).cuda())
        ctx.run_target(desc, P.Target(min_psnr_db=30.0, max_strength=19), 2)
        assert call(ctx, 0, freq, rank) == L.PNGLOSS_INVALID_ARGUMENT                               # a search leaves no batch to index
        with pytest.raises(RuntimeError):
            ctx.original_tables(0)
    finally:
        ctx.close()


def test_tables_follow_the_chunks_of_a_split_host_window(monkeypatch):
    """a host window in two chunks, the second on a peer context: image i's tables are read from the context that ran it"""
    monkeypatch.setenv("PNGLOSS_HIP_SPLIT", "2")
    specs = [(64, 2, "noise", "rgba"), (13, 7, "four", "rgb"), (12, 7, "noise", "graya"), (8, 5, "four", "gray"), (13, 7, "noise", "rgb"), (64, 2, "four", "graya")]
    want = [R.expected(*s) for s in specs]
    assert len({w[3].tobytes() for w in want}) == 6                        # distinct tables: a wrong chunk mapping shows
    ctx = P.HipContext()
    try:
        outs, filts, res = ctx.run_host([R.content(*s) for s in specs], 19, 2)
        got = [ctx.original_tables(i) for i in range(6)]
        engines = [ctx.engine_info(i)["engine"] for i in range(6)]
        with pytest.raises(RuntimeError):
            ctx.original_tables(6)
        assert P.hip_lib().pngloss_hip_last_engine_ms(ctx._ctx) >= 0
    finally:
        ctx.close()
    assert ROWS not in engines
    for i, (w, g) in enumerate(zip(want, got)):
        assert res[i]["status"] == 0 and np.array_equal(outs[i], w[0]) and np.array_equal(filts[i], w[1]), specs[i]
        assert np.array_equal(g[0], w[3]) and np.array_equal(g[1], w[4]), specs[i]


# ------------------------------------------------------------------------------------------------ batches of 65 540 images

SPLIT_N = 65540
SLOT, SLOT_FILTERS = 32, 24            # a device slot per image: up to 3 x 2 pixels, then its two filter bytes


def _pool():
    """seven images of 1 x 1 to 3 x 2 pixels over the four classes and one without pixels, read-only; image i of the batch is pool[i % 7]"""
    rng = np.random.default_rng(61)
    out = []
    for (w, h), cls in (((1, 1), "rgba"), ((2, 1), "rgb"), ((3, 1), "graya"), ((1, 2), "gray"), ((2, 2), "rgba"), ((3, 2), "rgb"), ((0, 0), "gray")):
        img = rng.integers(0, 200, (h, w, 4), dtype=np.uint8)
        if img.size:
            img[0, 0] = (10, 20, 30, 40)                                 # neither gray nor opaque before the class is forced
        img = U.as_pixel_class(img, cls)
        img.setflags(write=False)
        out.append((cls, img))
    return out


def _pool_expected(pool, s):
    """per pool image (slot bytes after the run, result (status, bpp), original_frequency, ranks) from the oracle at strength s, bleed 2"""
    want = []
    for cls, img in pool:
        h, w = img.shape[:2]
        slot = np.zeros(SLOT, np.uint8)
        bpp = R.BPP_OF_CLASS[cls]
        if img.size:
            out, filt = U.run_port(np.array(img), s, 2)
            slot[: img.size] = out.reshape(-1)
            slot[SLOT_FILTERS: SLOT_FILTERS + h] = filt
            freq = R.oracle_orig_tables(R.packed(img, bpp))
        else:
            freq = np.zeros((5, 256), np.uint32)
        want.append((slot, (0, bpp), freq, R.rank_rule(freq)))
    return want


def _run_device_pool(ctx, pool, s):
    """the 65 540 images in one device buffer, a slot each: (slots after the run (n, SLOT), (n, 2) array of status and bpp)"""
    import torch
    n = SPLIT_N
    slots = np.zeros((7, SLOT), np.uint8)
    for k, (_, img) in enumerate(pool):
        slots[k, : img.size] = img.reshape(-1)
    host = slots[np.arange(n) % 7]
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr()
    assert base % 16 == 0
    shape = [(img.shape[1], img.shape[0]) for _, img in pool]
    desc = [((base + i * SLOT, base + i * SLOT + SLOT_FILTERS) if shape[i % 7][0] else (0, 0)) + shape[i % 7] for i in range(n)]
    res = ctx.run(desc, s, 2)
    torch.cuda.synchronize()
    return dev.cpu().numpy(), np.array([(r["status"], r["bpp"]) for r in res], np.int64)


def _check_device_pool(ctx, s, engine):
    pool = _pool()
    n = SPLIT_N
    assert n > R.MAX_IMAGES == 65535 and n - R.MAX_IMAGES < len(pool) == 7 and R.slice_images(n, R.MAX_IMAGES) == 5
    want = _pool_expected(pool, s)
    assert len({w[0].tobytes() for w in want}) == 7 and sorted({w[1][1] for w in want}) == [1, 2, 3, 4]
    got, res = _run_device_pool(ctx, pool, s)
    which = np.arange(n) % 7
    want_slots, want_res = np.stack([w[0] for w in want])[which], np.array([w[1] for w in want], np.int64)[which]
    bad = np.flatnonzero((got != want_slots).any(axis=1) | (res != want_res).any(axis=1))
    assert not bad.size, "%d images differ, the first at %s; around the end of the first launch: %s" % (
        bad.size, bad[:8].tolist(), {i: (got[i].tolist(), res[i].tolist(), want_slots[i].tolist(), want_res[i].tolist()) for i in range(65533, 65538)})
    for i in list(range(7)) + list(range(n - 12, n)):
        assert ctx.engine_info(i)["engine"] == engine, i
        freq, rank = ctx.original_tables(i)
        assert np.array_equal(freq, want[i % 7][2]), i
        assert (rank is None) if engine == ROWS else np.array_equal(rank, want[i % 7][3]), i


def test_more_images_than_one_launch_takes_device_form(wg_ctx):
    """65 540 images at (19, 2) on the workgroup engine: pl_classify, pl_repack, pl_hist and pl_unpack have the batch in gridDim.y and take 65 535
    a launch, so the last five are a second launch of each, which must start at its own jobs"""
    _check_device_pool(wg_ctx, 19, WG)


def test_more_images_than_one_launch_takes_strength_0():
    """the same at strength 0, nothing pinned: here pl_rows_stats is the launch that is sliced"""
    ctx = P.HipContext()
    try:
        _check_device_pool(ctx, 0, ROWS)
    finally:
        ctx.close()


def test_more_images_than_one_launch_takes_host_form_with_streams():
    """run_host_zlib at strength 0: a deflate window is not cut into chunks, so pl_emit_classify, pl_emit_rows and the deflate's dfl_pack, dfl_near and
    dfl_keys (a deflate block per image) see all 65 540.  Colour type and stream of every image are those of its pool image run alone and of the CPU
    run of the encoder core on the restated scanlines."""
    pool = _pool()
    n = SPLIT_N
    imgs = [img for _, img in pool]
    ctx = P.HipContext()
    try:
        alone = [ctx.run_host_zlib([img], 0, 2)[2][0] for img in imgs]
        outs, filts, streams, res = ctx.run_host_zlib([imgs[i % 7] for i in range(n)], 0, 2, want_results=True)
    finally:
        ctx.close()
    for (cls, img), (ctype, z, blocks) in zip(pool, alone):
        if not img.size:
            assert z == b""
            continue
        _, filt = U.run_port(np.array(img), 0, 2)
        ct, ids, rows = U.png_scanlines_reference(img, filt)
        assert ctype == ct == {"rgba": 6, "rgb": 2, "graya": 4, "gray": 0}[cls]
        assert z == U.deflate_host(np.concatenate([ids[:, None], rows], axis=1).tobytes())[0], cls
    assert len({z for _, z, _ in alone}) == 7
    bad = [i for i in range(n) if streams[i] != alone[i % 7] or res[i]["status"] != 0 or not np.array_equal(outs[i], imgs[i % 7])]
    assert not bad, "%d images differ, the first at %s; around the end of the first launch: %s" % (
        len(bad), bad[:8], {i: (streams[i], alone[i % 7]) for i in range(65533, 65538)})

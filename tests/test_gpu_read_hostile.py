"""The device inflater on hostile streams (pngloss_hip_png_decode_batch_device_z; pl_inflate_core.h, one wave per stream): the hand-built corpus of
tests/util_inflate.py -- the streams the sanitized CPU programs of tests/test_inflate_hostile_host.py ran clean -- as gray 8-bit images one row high,
so that a stream's payload IS the scanline (width = payload - 1, first byte 0: filter type none).  What a stream must do is what zlib does with it;
what its ordinary neighbours in the batch must give are their golden pixels.  Nothing here comes from the CPU harness of the core under test: this
is what checks the halves of the core only the device has (the placement of literal runs by lane counts, the pending lanes of a match, the lane
reads of the chain, the wave sums of the Adler-32)."""
import struct
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U
from tests import util_inflate as Z
from tests.test_png_read import _device_bytes


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def _gray_file(width):
    """a gray 8-bit file one row high (its own image data is never used: the tests hand the streams in)"""
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, 1, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(bytes(width + 1), 1)) + _chunk(b"IEND", b"")


def _expanded(scanline):
    g = np.frombuffer(scanline, np.uint8)[1:]
    return np.stack([g, g, g, np.full_like(g, 255)], axis=1)


@pytest.mark.gpu
def test_stored_final_block_with_its_trailer_across_the_input_stage():
    """A final stored block ends wherever the 4 KB input stage does: the Adler-32 trailer 4, 3, 2, 1 or 0 bytes inside the stage, at the first and at
    the third turnover of the stage (streams of 4096..4100 and 12288..12292 bytes), in one batch.  Every one inflates: status 0, the payload's pixels.
    (Before the trailer was read across the stage's end, the eight streams with fewer than four bytes inside came back with status 25.)"""
    cases = [c for c in Z.corpus() if c[0].startswith("stored_final_trailer_")]
    assert sorted(len(c[1]) for c in cases) == [4096 * t + k for t in (1, 3) for k in range(5)]
    want = [Z.zlib_accepts(z, expect) for _, z, expect, _ in cases]
    assert all(w is not None and w[0] == 0 for w in want)
    ctx = P.HipContext()
    fr, st, rc = ctx.png_decode_device_z([_gray_file(expect - 1) for _, _, expect, _ in cases], zstreams=[z for _, z, _, _ in cases])
    assert rc == 0 and st == [0] * len(cases), (rc, st)
    for (name, _, expect, _), w, (ptr, width, height) in zip(cases, want, fr):
        assert (width, height) == (expect - 1, 1)
        assert np.array_equal(_device_bytes(ptr, width * 4).reshape(width, 4), _expanded(w)), name
    ctx.close()


@pytest.mark.gpu
def test_hand_built_corpus_between_ordinary_files():
    """Every hand-built stream that fits an image (two bytes and more: one pixel), with two ordinary fixture files between every two of them, in one
    batch: status 0 exactly where zlib accepts the stream and 25 elsewhere, the call's return code 25, accepted frames equal to zlib's bytes expanded,
    the neighbours equal to their golden pixels."""
    cases = [c for c in Z.corpus() if c[2] >= 2]
    assert len(cases) >= 700
    small = [f for f in U.png_read_fixtures() if f[2].shape[0] * f[2].shape[1] <= 4096]
    assert len(small) >= 30
    files, zs, expected = [], [], []                   # expected: None (refused), or the frame as (H, W, 4)
    for k, (name, z, expect, _) in enumerate(cases):
        w = Z.zlib_accepts(z, expect)
        assert w is None or w[0] == 0, name
        files.append(_gray_file(expect - 1)); zs.append(z); expected.append(None if w is None else _expanded(w).reshape(1, expect - 1, 4))
        for f in (small[(2 * k) % len(small)], small[(2 * k + 1) % len(small)]):
            files.append(f[1]); zs.append(L.parse_png(f[1])["zstream"]); expected.append(f[2])
    assert sum(e is None for e in expected) >= 300 and sum(e is not None for e in expected[::3]) >= 300
    ctx = P.HipContext()
    fr, st, rc = ctx.png_decode_device_z(files, zstreams=zs)
    assert rc == 25
    label = lambda i: cases[i // 3][0] if i % 3 == 0 else "neighbour %d of %s" % (i % 3, cases[i // 3][0])
    wrong = [(label(i), s) for i, (s, e) in enumerate(zip(st, expected)) if s != (25 if e is None else 0)]
    assert not wrong, wrong[:10]
    for i, (e, (ptr, width, height)) in enumerate(zip(expected, fr)):
        if e is not None:
            assert (height, width) == e.shape[:2], label(i)
            assert np.array_equal(_device_bytes(ptr, width * height * 4).reshape(height, width, 4), e), label(i)
    ctx.close()

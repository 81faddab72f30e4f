"""CPU tests of the deflate's measure-only mode (no GPU compute): both block encoders of pngloss_amd/csrc/pl_deflate_core.h / pl_deflate_coop.h run
in both modes on the CPU under the sanitizers (tests/c/deflate_measure_host.cpp).  Per block the measuring mode's record equals the writing mode's;
folded per image, the way the kernel dfl_sizes folds it, it equals the length and the Adler-32 of the stream the writing mode wrote.  The measuring
mode gets no output buffer at all."""
import zlib

import numpy as np
import pytest

from tests import util as U
from tests import util_size as S
from tests import util_target as T

TEAMS = (0, 1, 2, 7, 64)          # 0: the one-thread encoder; else dfl_encode_block_coop with that many threads
SMALL_BLOCK = 4096


def _inputs():
    rng = np.random.default_rng(5)
    text = (np.arange(3 * SMALL_BLOCK) % 251 * 7 % 256).astype(np.uint8).tobytes()
    out = [("empty", b"", SMALL_BLOCK), ("one_byte", b"\x07", SMALL_BLOCK), ("constant", bytes(20000), SMALL_BLOCK),
           ("noise", rng.integers(0, 256, 3 * SMALL_BLOCK + 17, dtype=np.uint8).tobytes(), SMALL_BLOCK),
           ("noise_one_block", rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), 262144)]     # stored form in two 65535-byte chunks
    for d in (-1, 0, 1):
        out.append(("border%+d" % d, text[: SMALL_BLOCK + d], SMALL_BLOCK))
        out.append(("border2%+d" % d, text[: 2 * SMALL_BLOCK + d], SMALL_BLOCK))
    for s in (0, 19, 85):                                        # oracle scanline streams: the bytes the product deflates
        _, o, f, _, _ = T.oracle_probe(130, 24, 0, s)
        out.append(("scanlines_s%d" % s, S.scanline_bytes(o, f)[1], SMALL_BLOCK))
    _, o, f, _, _ = T.oracle_probe(64, 16, 3, 19)
    out.append(("scanlines_product_block", S.scanline_bytes(o, f)[1], 262144))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_measure_host")
    exe = S.build_deflate_measure_host(d)
    inputs = _inputs()
    cmds = []
    for name, data, block in inputs:
        (d / (name + ".in")).write_bytes(data)
        cmds.append("D %s %s %d %s" % (d / (name + ".in"), d / (name + ".z"), block, " ".join(map(str, TEAMS))))
    lines = S.run_host(exe, d, cmds)
    return d, inputs, lines


def _parse(part):
    v = [int(x) for x in part.split()]
    nb = v[0]
    blocks = [(tuple(v[6 + 10 * b: 11 + 10 * b]), tuple(v[11 + 10 * b: 16 + 10 * b])) for b in range(nb)]
    return nb, v[1], v[2], tuple(v[3:6]), blocks


def test_every_block_measures_what_it_writes_and_the_fold_is_the_stream(answers):
    d, inputs, lines = answers
    kinds_seen = set()
    for (name, data, block), line in zip(inputs, lines):
        parts = line.split("|")
        assert len(parts) == len(TEAMS)
        streams = set()
        for team, part in zip(TEAMS, parts):
            nb, rec_bytes, rec_adler, rec_kinds, blocks = _parse(part)
            assert nb == (len(data) + block - 1) // block, (name, team)
            for b, (w, m) in enumerate(blocks):
                assert w == m, (name, team, b, w, m)             # bytes, kind, tokens, adler_a, adler_b
                kinds_seen.add(w[1])
            z = (d / ("%s.z.%d" % (name, team))).read_bytes()
            streams.add(z)
            assert rec_bytes == len(z), (name, team)
            assert sum(rec_kinds) == nb and rec_kinds == tuple(sum(1 for w, _ in blocks if w[1] == k) for k in range(3)), (name, team)
            if data:
                assert rec_adler == zlib.adler32(data) == int.from_bytes(z[-4:], "big"), (name, team)
                assert zlib.decompress(z) == data, (name, team)
            else:
                assert z == b"" and rec_adler == 1 and rec_bytes == 0
        assert len(streams) == 1, name                           # every team size writes the same stream
    assert kinds_seen == {0, 1, 2}                               # stored, fixed and dynamic blocks were all measured


def test_the_product_block_size_agrees_with_the_python_side_chain(answers):
    """the stream of the harness, product settings, is the stream U.deflate_host (the existing CPU run of the encoder) gives: the sizes the pinned
    table is made of are sizes of this encoder"""
    d, inputs, lines = answers
    for name in ("scanlines_product_block", "noise_one_block"):
        data = next(x[1] for x in inputs if x[0] == name)
        want, _ = U.deflate_host(data)
        assert (d / (name + ".z.0")).read_bytes() == want and (d / (name + ".z.64")).read_bytes() == want

"""GPU tests of the option "indexed" (include/pngloss_hip.h, "Indexed-colour streams"): pngloss_hip_optimize_batch_host_zlib with the option on against
the numpy restatement of tests/util_index.py applied to the pixels the same call returned, against the call with the option off, and against the CPU
run of the device's deflate encoder (tests/util.py:deflate_host) on the restated index rows.  Then the suite images the feature was proposed on,
the command line switch, and the multi-context form.  The shapes of X.device_shapes() take the loops of pl_index_rows and pl_index_count past their
first trip; for them the decision and both streams are also worked out on the CPU alone."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_index as X

pytestmark = pytest.mark.gpu

SHAPES = X.shapes()
NAMES = list(SHAPES)
STRENGTHS = (0, 19)
OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")


def _call(ctx, images, strength, indexed):
    """(outs, filters, streams, results, palettes): palettes None with the option off"""
    ctx.set_option("indexed", "on" if indexed else "off")
    outs, filts, zs, res = ctx.run_host_zlib([a.copy() for a in images], strength, 2, want_results=True)
    pal = [ctx.palette(i).as_dict() for i in range(len(images))] if indexed else None
    return outs, filts, zs, res, pal


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """strength -> (off, on): ONE batch of every shape -- eligible, non-eligible and empty images mixed -- with the option off and on"""
    images = [SHAPES[n] for n in NAMES]
    return {s: (_call(ctx, images, s, False), _call(ctx, images, s, True)) for s in STRENGTHS}


def _check(off, on, i, what):
    (o_outs, o_filts, o_zs, o_res, _), (outs, filts, zs, res, pals) = off, on
    # pixels, filters and results do not depend on the option
    assert np.array_equal(outs[i], o_outs[i]) and np.array_equal(filts[i], o_filts[i]) and res[i] == o_res[i], what
    want, pal = X.restate(outs[i]), pals[i]
    ctype, stream, blocks = zs[i]
    assert pal["colors"] == want["colors"], what
    assert pal["truecolor_bytes"] == len(o_zs[i][1]), what
    kept = False
    if want["eligible"]:
        indexed_stream = U.deflate_host(want["scanlines"])[0]
        print(what, "colours", want["colors"], "T", pal["truecolor_bytes"], "I", pal["indexed_bytes"], "I on the CPU", len(indexed_stream))
        assert pal["indexed_bytes"] == len(indexed_stream), what
        kept = X.keep_indexed(True, len(indexed_stream), len(o_zs[i][1]), want["entries"], want["trns_entries"])
    else:
        assert pal["indexed_bytes"] == 0, what
    if kept:
        assert ctype == 3, what
        assert (pal["entries"], pal["trns_entries"], pal["plte"], pal["trns"]) == (want["entries"], want["trns_entries"], want["plte"], want["trns"]), what
        assert zlib.decompress(stream) == want["scanlines"], what
        assert stream == indexed_stream and len(stream) + X.overhead(pal["entries"], pal["trns_entries"]) < pal["truecolor_bytes"], what
    else:
        # truecolour: byte for byte the stream of the call with the option off
        assert (ctype, stream, blocks) == o_zs[i] and ctype in (0, 2, 4, 6, -1), what
        assert (pal["entries"], pal["trns_entries"], pal["plte"], pal["trns"]) == (0, 0, b"", b""), what
    return kept


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("name", NAMES)
def test_shape_against_the_restatement(runs, name, strength):
    off, on = runs[strength]
    i = NAMES.index(name)
    kept = _check(off, on, i, f"{name} at strength {strength}")
    if name in ("257x1_257_colours",) and strength == 0:
        assert on[4][i]["colors"] == 257 and not kept
    if name == "empty":
        assert on[4][i] == dict(entries=0, trns_entries=0, plte=b"", trns=b"", truecolor_bytes=0, indexed_bytes=0, colors=0) and on[2][i][1] == b""


def test_the_batch_mixes_both_answers(runs):
    """at strength 0 the pixels are the inputs: the shapes that must be eligible are, and some image of the batch goes each way"""
    off, on = runs[0]
    colors = {n: on[4][NAMES.index(n)]["colors"] for n in NAMES}
    assert colors["16x16_256_colours"] == 256 and colors["300x200_scattered_256"] == 256 and colors["257x1_257_colours"] == 257
    assert colors["1x1"] == 1 and colors["130x9_five_colours"] == 5 and colors["256_alphas_of_one_rgb"] == 256 and colors["colliding_hash"] == 40
    ctypes = [z[0] for z in on[2]]
    assert 3 in ctypes and any(c in (0, 2, 4, 6) for c in ctypes)
    assert on[2][NAMES.index("300x200_scattered_256")][0] == 3          # 60 000 random indices against 180 000 random bytes


def test_single_image_calls_equal_the_batch(ctx, runs):
    for name in ("130x9_five_colours", "257x1_257_colours"):
        i = NAMES.index(name)
        one = _call(ctx, [SHAPES[name]], 0, True)
        assert one[2][0] == runs[0][1][2][i] and one[4][0] == runs[0][1][4][i], name


# ---- the loops past one trip (X.device_shapes): rows past the 512 workgroups of an image, pixels past the 1024 of one pass, chunks past the
# workgroups of the count kernel ----

TRIPS = ["3x1100_five_colours", "4099x3_five_colours", "1030x520_256_colours"]
LAST_PIXEL = ["257th_in_the_last_pixel", "257th_in_the_first_pixel", "256th_in_the_last_pixel"]


@pytest.fixture(scope="module")
def device():
    shapes = X.device_shapes()
    assert list(shapes) == TRIPS + LAST_PIXEL
    return shapes


@pytest.fixture(scope="module")
def on_the_cpu(device):
    """name -> (kept, indexed stream or None, truecolour stream): the decision and both streams of the unchanged pixels from the restatements
    and the CPU run of the encoder alone -- nothing of it comes from the library"""
    out = {}
    for name, img in device.items():
        pixels, flags = U.run_port(img, 0, 2)
        assert np.array_equal(pixels, img)                                  # strength 0 changes no pixel
        _, ids, rows = U.png_scanlines_reference(img, flags)
        truecolor = U.deflate_host(np.concatenate([ids[:, None], rows], axis=1).tobytes())[0]
        want = X.restate(img)
        indexed = U.deflate_host(want["scanlines"])[0] if want["eligible"] else None
        kept = X.keep_indexed(want["eligible"], len(indexed or b""), len(truecolor), want.get("entries", 0), want.get("trns_entries", 0))
        print(name, "colours", want["colors"], "I", len(indexed or b""), "T", len(truecolor), "kept", kept)
        out[name] = (kept, indexed, truecolor)
    return out


@pytest.fixture(scope="module")
def alone(ctx, device):
    """name -> (off, on): every device shape in a call of its own, at strength 0"""
    return {name: (_call(ctx, [img], 0, False), _call(ctx, [img], 0, True)) for name, img in device.items()}


@pytest.mark.parametrize("name", TRIPS)
def test_rows_and_pixels_past_one_trip(device, on_the_cpu, alone, name):
    img = device[name]
    h, w = img.shape[:2]
    if name == "3x1100_five_colours":           # rows 512..1023 a second trip of their workgroup, rows 1024..1099 a ragged third
        assert h > 2 * X.ROW_BLOCKS and h % X.ROW_BLOCKS and w < 4
    if name == "4099x3_five_colours":           # four passes of 1024 pixels and a tail of three
        assert w == 4 * X.ROW_PASS + 3 and w % 4 == 3 and h < X.ROW_BLOCKS
    if name == "1030x520_256_colours":          # both loops at once, and a full table
        assert h > X.ROW_BLOCKS and w > X.ROW_PASS and X.restate(img)["colors"] == 256
    cpu_kept, indexed, truecolor = on_the_cpu[name]
    assert cpu_kept, name                       # the indexed stream is the one that comes back: its bytes are compared, not only its length
    off, on = alone[name]
    assert _check(off, on, 0, name)
    assert on[2][0] == (3, indexed, on[2][0][2]) and off[2][0][1] == truecolor, name
    assert np.array_equal(on[0][0], img), name


@pytest.mark.parametrize("name", LAST_PIXEL)
def test_the_deciding_colour_in_one_pixel(device, on_the_cpu, alone, name):
    """59 chunks over the workgroups of pl_index_count: the 257th colour, or the 256th, only in the last pixel of the last chunk (or the first
    of the first) -- where the early exit, which re-reads the counter before each chunk and each insertion, decides eligibility"""
    img = device[name]
    assert img.shape[:2] == (200, 300) and -(-300 * 200 // 1024) == 59
    cpu_kept, indexed, truecolor = on_the_cpu[name]
    off, on = alone[name]
    kept = _check(off, on, 0, name)
    pal = on[4][0]
    assert kept == cpu_kept and off[2][0][1] == truecolor and np.array_equal(on[0][0], img), name
    if name.startswith("257th"):
        assert X.restate(img)["colors"] == 257 and not kept
        assert pal["colors"] == 257 and pal["indexed_bytes"] == 0 and on[2][0] == off[2][0], name
    else:
        assert X.restate(img)["colors"] == 256 and kept
        assert pal["colors"] == 256 and pal["entries"] == 256 and len(pal["plte"]) == 3 * 256 and on[2][0][:2] == (3, indexed), name


def test_the_device_shapes_in_one_batch_equal_each_alone(ctx, device, alone):
    names = list(device) + ["1x1", "empty"]
    images = [device[n] for n in device] + [SHAPES["1x1"], np.zeros((0, 0, 4), np.uint8)]
    off, on = _call(ctx, images, 0, False), _call(ctx, images, 0, True)
    for i, (name, img) in enumerate(zip(names, images)):
        _check(off, on, i, f"{name} in the batch")
        one_off, one_on = alone[name] if name in alone else (_call(ctx, [img], 0, False), _call(ctx, [img], 0, True))
        for batch, one in ((off, one_off), (on, one_on)):
            assert np.array_equal(batch[0][i], one[0][0]) and np.array_equal(batch[1][i], one[1][0]) and batch[2][i] == one[2][0] and batch[3][i] == one[3][0], name
        assert on[4][i] == one_on[4][0], name
    assert [z[0] for z in on[2]][:6] == [3, 3, 3] + [off[2][3][0], off[2][4][0], 3] and on[2][-1][1] == b""


def test_accessor_rules(ctx):
    img = SHAPES["130x9_five_colours"]
    _call(ctx, [img], 0, False)
    with pytest.raises(RuntimeError):
        ctx.palette(0)                                  # the last batch ran with the option off
    _call(ctx, [img], 0, True)
    assert ctx.palette(0).colors == 5
    with pytest.raises(RuntimeError):
        ctx.palette(1)                                  # out of range
    ctx.run_host([img.copy()], 0, 2)                    # option still on, but the call returns no stream: nothing to report
    with pytest.raises(RuntimeError):
        ctx.palette(0)
    with pytest.raises(RuntimeError):
        ctx.set_option("indexed", "maybe")
    ctx.set_option("indexed", "off")


@pytest.fixture(scope="module")
def suite():
    g = U.load_npz("suite_inputs.npz")
    return {n: g[n] for n in ("tux", "barbara", "lena")}


def test_suite_images_at_strength_0(ctx, suite):
    """tux, a palette file that used to come out 2.4 times its size, goes indexed; a gray image and a photograph stay what they were"""
    names = list(suite)
    images = [suite[n] for n in names]
    off, on = _call(ctx, images, 0, False), _call(ctx, images, 0, True)
    kept = {n: _check(off, on, i, n) for i, n in enumerate(names)}
    pals = dict(zip(names, on[4]))
    ctypes = dict(zip(names, (z[0] for z in on[2])))
    assert kept["tux"] and ctypes["tux"] == 3 and pals["tux"]["colors"] == 194
    assert not kept["barbara"] and ctypes["barbara"] == 0 and pals["barbara"]["colors"] == 234 and pals["barbara"]["indexed_bytes"] > 0
    assert not kept["lena"] and ctypes["lena"] == 2 and pals["lena"]["colors"] == 257 and pals["lena"]["indexed_bytes"] == 0


@pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")
def test_tool_writes_tux_as_a_smaller_palette_file(tmp_path, suite):
    from PIL import Image
    src = str(tmp_path / "tux.png")
    Image.fromarray(suite["tux"], "RGBA").save(src)
    files = {}
    for tag, args in (("plain", ["--gpu-deflate"]), ("indexed", ["--indexed", "-v"]), ("capped", ["--indexed", "--skip-if-larger"])):
        out = str(tmp_path / f"tux-{tag}.png")
        r = subprocess.run([OUR_CLI, "-f", "-s", "0", "-o", out, src] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1000:]
        files[tag] = open(out, "rb").read()
        if tag == "indexed":
            assert "  indexed: 194 colours, " in r.stderr
    plain, indexed = files["plain"], files["indexed"]
    assert files["capped"] == indexed
    assert dict(X.chunks_of(plain))[b"IHDR"][8:10] == b"\x08\x06" and dict(X.chunks_of(indexed))[b"IHDR"][8:10] == b"\x08\x03"
    assert len(indexed) < len(plain)
    a, b = (np.asarray(Image.open(io.BytesIO(f)).convert("RGBA")) for f in (plain, indexed))
    assert np.array_equal(a, b) and np.array_equal(b, suite["tux"])
    # the written file is what the library decided on: PLTE and tRNS are the restatement's
    want = X.restate(suite["tux"])
    ch = dict(X.chunks_of(indexed))
    assert ch[b"PLTE"] == want["plte"] and ch.get(b"tRNS", b"") == want["trns"] and zlib.decompress(ch[b"IDAT"]) == want["scanlines"]


def test_multi_form_follows_the_image():
    """two contexts on device 0: the record of images[i] comes from whichever context image i went to"""
    rng = np.random.default_rng(2)
    names = ["130x9_five_colours", "300x200_scattered_256", "16x16_256_colours", "one_translucent", "257x1_257_colours"]
    images = [SHAPES[n] for n in names] + [rng.integers(0, 256, (150, 260, 4), dtype=np.uint8)]
    owners = P.multi_split([(a.shape[1], a.shape[0]) for a in images], 2)
    assert set(owners) == {0, 1}
    m = P.HipMulti("0,0")
    try:
        with pytest.raises(RuntimeError):
            m.palette(0)
        m.set_option("indexed", "on")
        outs, filts, res, zs = m.run_host_zlib([a.copy() for a in images], 0, 2)
        pals = [m.palette(i).as_dict() for i in range(len(images))]
        with pytest.raises(RuntimeError):
            m.palette(len(images))
        m.set_option("indexed", "off")
        o_outs, o_filts, o_res, o_zs = m.run_host_zlib([a.copy() for a in images], 0, 2)
    finally:
        m.close()
    off, on = (o_outs, o_filts, o_zs, o_res, None), (outs, filts, zs, res, pals)
    kept = [_check(off, on, i, f"image {i}") for i in range(len(images))]
    assert kept[1] and not kept[4] and not kept[5] and pals[5]["colors"] == 257

"""GPU tests of the option "index_depth" (include/pngloss_hip_index_depth.h): pngloss_hip_optimize_batch_host_zlib at strength 0 with the option at
"8", "auto" and "min" against the numpy restatement of tests/util_index_depth.py -- the packed scanlines, the rule that names the stream to keep
--, against the CPU run of the device's deflate encoder on the restated rows (tests/util.py:deflate_host: the size of a candidate is checked even
where its stream was not kept), and against the call with "indexed" off for every truecolour stream.  Then the read side's decode of the packed
streams on the device, the multi form, and the streams behind the quantiser."""
import zlib

import numpy as np
import pytest

import pngloss_amd as P
from tests import util as U
from tests import util_index as X
from tests import util_index_depth as D

pytestmark = pytest.mark.gpu


def _records(obj, n):
    return [obj.palette(i).as_dict() for i in range(n)], [obj.index_depth(i).as_dict() for i in range(n)]


def _call(ctx, images, mode, strength=0):
    """dict(outs, zs, pals, recs) of one zlib call; mode None: "indexed" off; "unset": on, "index_depth" never touched"""
    ctx.set_option("indexed", "off" if mode is None else "on")
    if mode not in (None, "unset"):
        ctx.set_option("index_depth", mode)
    outs, _, zs = ctx.run_host_zlib([a.copy() for a in images], strength, 2)
    pals, recs = _records(ctx, len(images)) if mode is not None else (None, None)
    return dict(outs=outs, zs=zs, pals=pals, recs=recs)


@pytest.fixture(scope="module")
def ctx():
    c = P.HipContext()
    yield c
    c.close()


def _check(mode, img, run, off, i, what):
    """image i of a run under `mode` against the restatement; `off`: the same batch with "indexed" off.  Returns the bit depth kept."""
    out, (ctype, stream, blocks), pal, rec = run["outs"][i], run["zs"][i], run["pals"][i], run["recs"][i]
    assert np.array_equal(out, img) and np.array_equal(off["outs"][i], img), what          # strength 0 changes no pixel
    want = X.restate(img)
    T = len(off["zs"][i][1])
    colors = want["colors"]
    md = D.min_depth(colors) if want["eligible"] else 0
    has8, hasp = bool(md) and (mode != "min" or md == 8), bool(md) and mode != "8" and md < 8
    I8 = len(U.deflate_host(D.scanlines(want["rows"], 8))[0]) if has8 else 0
    Ip = len(U.deflate_host(D.scanlines(want["rows"], md))[0]) if hasp else 0
    print(what, "mode", mode, "colours", colors, "min_depth", md, "T", T, "I8", I8, "Ip", Ip, "record", rec, "kept", ctype, len(stream))
    assert pal["colors"] == colors and pal["truecolor_bytes"] == T, what
    assert (rec["min_depth"], rec["indexed8_bytes"], rec["packed_bytes"]) == (md, I8, Ip), what
    depth, candidate = D.choose(mode, colors, T, I8, Ip, want.get("trns_entries", 0))
    assert rec["bit_depth"] == depth and pal["indexed_bytes"] == candidate, what
    if depth:
        assert ctype == 3 and len(stream) == (I8 if depth == 8 else Ip), what
        assert zlib.decompress(stream) == D.scanlines(want["rows"], depth), what           # exactly the restated rows of that depth
        assert (pal["entries"], pal["trns_entries"], pal["plte"], pal["trns"]) == (want["entries"], want["trns_entries"], want["plte"], want["trns"]), what
        assert np.array_equal(D.pixels_of(zlib.decompress(stream), img.shape[1], img.shape[0], depth, pal["plte"], pal["trns"]), img), what
    else:
        assert (ctype, stream, blocks) == off["zs"][i] and ctype != 3, what                # byte for byte the truecolour stream
        assert (pal["entries"], pal["trns_entries"], pal["plte"], pal["trns"]) == (0, 0, b"", b""), what
    return depth


def _colours_image(colors, width, height, seed, translucent=0):
    """`colors` colours over width x height pixels, every one present; the first `translucent` of them not opaque"""
    rng = np.random.default_rng(seed)
    pal = D.opaque_colours(colors, seed + 500)
    pal[:translucent] = (pal[:translucent] & np.uint32(0x00FFFFFF)) | np.uint32(0x40000000)
    idx = rng.integers(0, colors, width * height)
    idx[:colors] = rng.permutation(colors)
    return X.from_words(pal[idx], width, height)


# ---- 1. the default path ----

def test_unset_and_8_are_the_same_call(ctx):
    shapes = X.shapes()
    names = ["1x1", "5x1", "130x9_five_colours", "16x16_256_colours", "257x1_257_colours", "one_translucent", "empty", "flat_70x30"]
    images = [shapes[n] for n in names] + [D.noise(2, 64, 64, 5), D.noise(16, 40, 30, 8)]
    fresh = P.HipContext()                                  # a context whose "index_depth" was never set
    try:
        unset = _call(fresh, images, "unset")
    finally:
        fresh.close()
    eight, off = _call(ctx, images, "8"), _call(ctx, images, None)
    assert unset["zs"] == eight["zs"] and unset["pals"] == eight["pals"] and unset["recs"] == eight["recs"]
    kept = [_check("8", img, eight, off, i, f"image {i}") for i, img in enumerate(images)]
    assert set(kept) == {0, 8}                              # the batch goes both ways, and never below 8 bits
    for (ctype, _, _), rec, pal in zip(eight["zs"], eight["recs"], eight["pals"]):
        assert rec["bit_depth"] == (8 if ctype == 3 else 0) and rec["packed_bytes"] == 0 and rec["indexed8_bytes"] == pal["indexed_bytes"]


# ---- 2. "min" ----

def test_min_mixes_every_depth_in_one_launch(ctx):
    """1, 2, 3, 4, 5, 16 and 17 colours at 7x3, 300 colours at 25x12 (7x3 has 21 pixels), and one pixel of the 2-colour palette at 1x1: the depths
    1, 2 and 4 go through one pl_index_pack launch, beside images that get no packed rows"""
    images = [_colours_image(c, 7, 3, 40 + c, translucent=1 if c == 3 else 0) for c in (1, 2, 3, 4, 5, 16, 17)]
    images += [_colours_image(300, 25, 12, 47), _colours_image(2, 7, 3, 42)[:1, :1].copy()]
    run, off = _call(ctx, images, "min"), _call(ctx, images, None)
    for i, img in enumerate(images):
        _check("min", img, run, off, i, f"image {i}")
    assert [r["min_depth"] for r in run["recs"]] == [1, 1, 2, 2, 4, 4, 8, 0, 1]
    assert all(r["indexed8_bytes"] == 0 for r in run["recs"][:6]) and run["recs"][6]["indexed8_bytes"] > 0 and run["recs"][6]["packed_bytes"] == 0


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_min_at_the_widths_where_the_lanes_change(ctx, depth):
    """a lane makes a dword from 32 / depth pixels, 256 lanes make a trip of 8192 / 4096 / 2048 pixels: widths 8, 9, 31, 32, 33 and one pixel past
    a trip, two rows each; and 5x600, past the 512 workgroups an image's rows get"""
    trip = D.trip_pixels(depth)
    assert trip == {1: 8192, 2: 4096, 4: 2048}[depth]
    colors = 1 << depth
    dims = [(w, 2) for w in (8, 9, 31, 32, 33, trip + 1)] + [(5, 600)]
    assert 600 > D.PACK_ROW_BLOCKS
    images = [_colours_image(colors, w, h, 60 + 7 * depth + k) for k, (w, h) in enumerate(dims)]
    run, off = _call(ctx, images, "min"), _call(ctx, images, None)
    kept = [_check("min", img, run, off, i, f"{dims[i]} at depth {depth}") for i, img in enumerate(images)]
    assert kept[5] == depth and kept[6] == depth            # the two large ones end packed: their streams were compared byte by byte above


# ---- 3. "auto" ----

@pytest.fixture(scope="module")
def auto_inputs():
    return {**D.noise_inputs(), **D.structured_inputs()}


def test_auto_keeps_the_candidate_the_rule_names(ctx, auto_inputs):
    names, images = list(auto_inputs), list(auto_inputs.values())
    run, off = _call(ctx, images, "auto"), _call(ctx, images, None)
    kept = {n: _check("auto", img, run, off, i, n) for i, (n, img) in enumerate(zip(names, images))}
    for i, n in enumerate(names):
        rec, pal = run["recs"][i], run["pals"][i]
        ov = X.overhead(pal["colors"], 0)
        print(n, "T", pal["truecolor_bytes"], "I8 + overhead", rec["indexed8_bytes"] + ov, "Ip + overhead", rec["packed_bytes"] + ov, "kept at", rec["bit_depth"])
        # from the record's own numbers: the smallest file, a tie to the earlier candidate
        costs = [(pal["truecolor_bytes"], 0), (rec["indexed8_bytes"] + ov, 8), (rec["packed_bytes"] + ov, rec["min_depth"])]
        assert rec["bit_depth"] == min(costs, key=lambda c: c[0])[1], n
        assert len(run["zs"][i][1]) == {0: pal["truecolor_bytes"], 8: rec["indexed8_bytes"]}.get(rec["bit_depth"], rec["packed_bytes"]), n
        if n.startswith("noise"):
            assert rec["bit_depth"] == rec["min_depth"] < 8, n
    # "auto" against "8": the same streams except where packed won
    eight = _call(ctx, images, "8")
    for i, n in enumerate(names):
        if kept[n] in (0, 8):
            assert run["zs"][i] == eight["zs"][i], n
        assert run["recs"][i]["indexed8_bytes"] == eight["recs"][i]["indexed8_bytes"], n


# ---- 4. round trip on the device ----

def test_packed_streams_decode_on_the_device(ctx, auto_inputs):
    images = list(auto_inputs.values()) + [_colours_image(2, 33, 5, 90), _colours_image(4, 9, 7, 91, translucent=2), _colours_image(16, 2049, 2, 92, translucent=1)]
    run = _call(ctx, images, "min")
    files, which = [], []
    for i, img in enumerate(images):
        rec, pal, (ctype, stream, _) = run["recs"][i], run["pals"][i], run["zs"][i]
        if 1 <= rec["bit_depth"] < 8:
            assert ctype == 3
            files.append(D.png_file(img.shape[1], img.shape[0], rec["bit_depth"], 3, stream, pal["plte"], pal["trns"]))
            which.append(i)
    assert {run["recs"][i]["bit_depth"] for i in which} == {1, 2, 4} and len(which) >= 6
    for i, got in zip(which, ctx.png_decode(files)):
        assert np.array_equal(got, images[i]), i


# ---- 5. the multi form, and the accessor's rules ----

def test_multi_form_follows_the_image():
    images = [D.noise(2, 64, 64, 5), X.shapes()["300x200_scattered_256"], D.noise(16, 40, 30, 8), X.shapes()["257x1_257_colours"], D.noise(4, 64, 64, 6),
              _colours_image(5, 130, 9, 95)]
    owners = P.multi_split([(a.shape[1], a.shape[0]) for a in images], 2)
    assert set(owners) == {0, 1}
    m = P.HipMulti("0,0")
    try:
        with pytest.raises(RuntimeError):
            m.index_depth(0)                                # nothing has run
        m.set_option("indexed", "on")
        m.set_option("index_depth", "auto")
        outs, _, _, zs = m.run_host_zlib([a.copy() for a in images], 0, 2)
        pals, recs = _records(m, len(images))
        with pytest.raises(RuntimeError):
            m.index_depth(len(images))
        m.run_host([a.copy() for a in images], 0, 2)        # a call without streams leaves nothing to report
        with pytest.raises(RuntimeError):
            m.index_depth(0)
        m.set_option("indexed", "off")
        o_outs, _, _, o_zs = m.run_host_zlib([a.copy() for a in images], 0, 2)
        with pytest.raises(RuntimeError):
            m.index_depth(0)                                # "indexed" off
        with pytest.raises(RuntimeError):
            m.set_option("index_depth", "4")
    finally:
        m.close()
    run, off = dict(outs=outs, zs=zs, pals=pals, recs=recs), dict(outs=o_outs, zs=o_zs)
    kept = [_check("auto", img, run, off, i, f"image {i}") for i, img in enumerate(images)]
    assert kept[0] == 1 and kept[4] == 2 and kept[1] == 8 and kept[3] == 0


def test_accessor_rules(ctx):
    img = D.noise(4, 64, 64, 6)
    _call(ctx, [img], None)
    with pytest.raises(RuntimeError):
        ctx.index_depth(0)                                  # the last batch ran with "indexed" off
    assert _call(ctx, [img], "min")["recs"][0]["bit_depth"] == 2
    with pytest.raises(RuntimeError):
        ctx.index_depth(1)                                  # out of range
    # a host window that runs in chunks returns no streams (a window with a deflate stage keeps its single pass): nothing to report in any chunk
    ctx.run_host([img.copy() for _ in range(16)], 0, 2)
    for i in (0, 15):
        with pytest.raises(RuntimeError):
            ctx.index_depth(i)
    for bad in ("4", "1", "on", "", "Auto"):
        with pytest.raises(RuntimeError):
            ctx.set_option("index_depth", bad)
    assert _call(ctx, [img], "unset")["recs"][0]["bit_depth"] == 2          # a refused value changes nothing: still "min"
    ctx.set_option("index_depth", "8")
    ctx.set_option("indexed", "off")


# ---- 6. behind the quantiser ----

@pytest.mark.parametrize("colors", [2, 4, 16])
def test_behind_the_quantiser(ctx, colors):
    y, x = np.mgrid[0:64, 0:96]
    gradient = np.stack([x * 255 // 95, y * 255 // 63, (x + y) * 255 // 158, np.full_like(x, 255)], axis=2).astype(np.uint8)
    m = P.HipMulti("0")
    try:
        outs, reports = m.quantize_host([gradient], colors)
    finally:
        m.close()
    quantised = outs[0]
    want = X.restate(quantised)
    assert 1 <= want["colors"] <= colors
    run, off = _call(ctx, [quantised], "auto"), _call(ctx, [quantised], None)
    depth = _check("auto", quantised, run, off, 0, f"gradient at {colors} colours")
    assert run["recs"][0]["min_depth"] == D.min_depth(want["colors"]) and depth in (0, 8, D.min_depth(want["colors"]))
    ctx.set_option("index_depth", "8")
    ctx.set_option("indexed", "off")

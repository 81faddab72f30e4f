"""GPU test of the tool's switch --index-depth (pngloss_amd/cli): the rose of the suite (70x46) through --colors with the switch at auto and min.  The
bit depth in IHDR is the one the -v line names, the file decodes -- with PIL, which shares no code with the writer -- to the pixels of the file
written without the switch, and a call without --colors or --indexed is refused before any file is touched."""
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from tests import util as U
from tests import util_index as X
from tests import util_index_depth as D

OUR_CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(OUR_CLI), reason="pngloss_amd/cli/pngloss is not built (no libpng headers)")]
Image = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def rose(tmp_path_factory):
    src = str(tmp_path_factory.mktemp("index_depth_cli") / "rose.png")
    with open(src, "wb") as fh:
        fh.write(U.load_npz("suite_png.npz")["rose"].tobytes())
    return src


def _run(src, out, args):
    r = subprocess.run([OUR_CLI, "-f", "-o", out, src] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    data = open(out, "rb").read()
    ch = dict(X.chunks_of(data))
    return data, ch, np.asarray(Image.open(io.BytesIO(data)).convert("RGBA")), r.stderr


def _check_file(ch, pixels, depth):
    """a palette file at `depth`: its scanlines are the restated rows of its pixels, its palette their colours in palette order"""
    want = X.restate(pixels)
    assert ch[b"IHDR"][8:10] == bytes([depth, 3]) and ch[b"PLTE"] == want["plte"] and ch.get(b"tRNS", b"") == want["trns"]
    assert zlib.decompress(ch[b"IDAT"]) == D.scanlines(want["rows"], depth)


@pytest.mark.parametrize("colors,mode", [(16, "auto"), (16, "min"), (2, "min")])
def test_tool_writes_the_depth_the_library_kept(tmp_path, rose, colors, mode):
    plain, plain_ch, plain_px, _ = _run(rose, str(tmp_path / "plain.png"), ["--colors", str(colors), "-v"])
    verbose = colors == 16
    data, ch, px, err = _run(rose, str(tmp_path / "depth.png"), ["--colors", str(colors), "--index-depth", mode] + (["-v"] if verbose else []))
    assert np.array_equal(px, plain_px)                                    # the same pixels as without the switch
    assert plain_ch[b"IHDR"][8] == 8                                       # ... which writes 8 bits whatever the colours
    md = D.min_depth(X.restate(px)["colors"])
    assert md == D.min_depth(colors)
    depth, ctype = ch[b"IHDR"][8], ch[b"IHDR"][9]
    lines = re.findall(r"^  index depth: .*\n", err, flags=re.M)
    print(colors, mode, "IHDR", depth, ctype, "bytes", len(data), "without the switch", len(plain), lines)
    if verbose:
        # the line is there exactly where the file went below 8 bits, and names the depth IHDR has
        assert len(lines) == (1 if ctype == 3 and depth < 8 else 0)
        if lines:
            m = re.match(r"  index depth: (\d) bits, (\d+) bytes of packed image data", lines[0])
            assert int(m.group(1)) == depth == md and int(m.group(2)) == len(ch[b"IDAT"])
            i8 = re.search(r"against (\d+) bytes at 8 bits", lines[0])
            assert lines[0] == D.report_line(dict(bit_depth=depth, indexed8_bytes=int(i8.group(1)) if i8 else 0, packed_bytes=len(ch[b"IDAT"])))
            assert bool(i8) == (mode == "auto")
            if i8 and plain_ch[b"IHDR"][9] == 3:
                assert int(i8.group(1)) == len(plain_ch[b"IDAT"])          # the 8-bit candidate is the stream of the file without the switch
    else:
        assert not lines
    if ctype == 3:
        _check_file(ch, px, depth)
        assert depth == (md if mode == "min" else depth) and depth in (md, 8)
        if depth < 8 and mode == "auto":                                   # ("min" may write the larger file: it does not look at the 8-bit one)
            assert len(data) < len(plain)
    else:
        assert data == plain or plain_ch[b"IHDR"][9] == 3                  # truecolour: the file of the call without the switch
    if mode == "min":
        assert ctype == 3 and depth == md                                  # rose at 16 and at 2 colours: the packed file beats truecolour


def test_switch_is_refused_without_a_palette_switch(tmp_path, rose):
    out = str(tmp_path / "never.png")
    for value in ("auto", "min", "8"):
        r = subprocess.run([OUR_CLI, "-f", "-o", out, rose, "--index-depth", value], capture_output=True, text=True, timeout=300)
        assert r.returncode == 4 and r.stderr == "--index-depth requires --indexed or --colors.\n", r.stderr
    r = subprocess.run([OUR_CLI, "-f", "-o", out, rose, "--colors", "16", "--index-depth", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 4 and r.stderr == "--index-depth requires auto, min or 8\n", r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")

"""CPU test of the container side of indexed colour: pngloss_amd/cli/png_stream_writer.c gets a palette, an optional tRNS payload and a zlib stream
of index rows made with Python's zlib (tests/c/index_write.c drives it, under the sanitizers); the file must decode -- with PIL, which shares no
code with the writer -- to the RGBA the palette and the indices stand for, its chunks must stand where libpng puts them, and
png_stream_file_size must account for the two new chunks."""
import io
import subprocess
import zlib

import numpy as np
import pytest

from tests import util_index as X

Image = pytest.importorskip("PIL.Image")


def _image(entries, trns_entries, width, height, seed):
    """an RGBA image of exactly `entries` colours, the first `trns_entries` of the palette order not opaque"""
    rng = np.random.default_rng(seed)
    rgb = rng.choice(1 << 24, entries, replace=False).astype(np.uint32)
    alpha = np.concatenate([rng.integers(0, 255, trns_entries), np.full(entries - trns_entries, 255)]).astype(np.uint32)
    if trns_entries == 256:
        alpha = np.arange(256, dtype=np.uint32) % 255                   # (two entries share alpha 0: their RGB differs)
    pal = rgb | (alpha << 24)
    w = np.concatenate([pal, rng.choice(pal, width * height - entries)]) if width * height > entries else pal[: width * height]
    return X.from_words(rng.permutation(w), width, height)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return X.build_index_write(tmp_path_factory.mktemp("index_write"))


def _write(exe, tmp_path, img, chunks="-", max_file_size=0):
    r = X.restate(img)
    assert r["eligible"]
    (tmp_path / "plte.bin").write_bytes(r["plte"])
    (tmp_path / "trns.bin").write_bytes(r["trns"])
    z = zlib.compress(r["scanlines"], 9)
    (tmp_path / "z.bin").write_bytes(z)
    out = tmp_path / "out.png"
    p = subprocess.run([exe, str(out), str(img.shape[1]), str(img.shape[0]), str(tmp_path / "plte.bin"), str(tmp_path / "trns.bin") if r["trns"] else "-",
                        str(tmp_path / "z.bin"), chunks, str(max_file_size)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    rc, written, meta, predicted = (int(v) for v in p.stdout.split())
    return r, z, out.read_bytes(), rc, written, meta, predicted


@pytest.mark.parametrize("entries,trns_entries,width,height,chunks", [
    (7, 0, 13, 5, "-"),             # no tRNS
    (7, 1, 13, 5, "-"),             # tRNS of length 1
    (256, 256, 32, 9, "-"),         # tRNS of 256 entries
    (1, 1, 1, 1, "-"),
    (40, 3, 31, 7, "b"),            # a passed-through chunk in front of PLTE ...
    (40, 3, 31, 7, "a"),            # ... and behind IDAT
    (40, 0, 31, 7, "bma"),
])
def test_palette_file_decodes_to_the_intended_pixels(exe, tmp_path, entries, trns_entries, width, height, chunks):
    img = _image(entries, trns_entries, width, height, seed=entries * 7 + trns_entries)
    r, z, data, rc, written, meta, predicted = _write(exe, tmp_path, img, chunks)
    assert rc == 0 and written == len(data) == predicted
    assert (r["entries"], r["trns_entries"]) == (entries, trns_entries)
    # decoded by PIL: exactly the intended RGBA
    got = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
    assert np.array_equal(got, img)
    # the container: IHDR says (8, 3); PLTE behind the gAMA / sRGB tags and the chunk from in front of it, tRNS right behind PLTE and only when
    # it has entries, both in front of the one IDAT; the other passed-through chunks in their places
    ch = X.chunks_of(data)
    tags = [t for t, _ in ch]
    want = [b"IHDR", b"gAMA", b"sRGB"] + ([b"prVt"] if "b" in chunks else []) + [b"PLTE"] + ([b"tRNS"] if trns_entries else []) + \
           ([b"miDl"] if "m" in chunks else []) + [b"IDAT"] + ([b"afTr"] if "a" in chunks else []) + [b"IEND"]
    assert tags == want
    body = dict(ch)
    assert body[b"IHDR"][8:10] == b"\x08\x03" and body[b"PLTE"] == r["plte"] and body[b"IDAT"] == z
    if trns_entries:
        assert body[b"tRNS"] == r["trns"] and len(body[b"tRNS"]) == trns_entries
    assert meta == sum(len(b) + 12 for t, b in ch if t in (b"prVt", b"miDl", b"afTr"))


def test_size_cap_judges_the_file_with_its_palette(exe, tmp_path):
    """--skip-if-larger hands the writer a cap: the PLTE and tRNS chunks count"""
    img = _image(200, 10, 40, 10, seed=3)
    r, z, data, rc, written, _, predicted = _write(exe, tmp_path, img)
    assert rc == 0 and written == predicted == len(data)
    assert predicted == 8 + 25 + 16 + 13 + 12 + len(z) + 12 + X.overhead(200, 10)
    assert _write(exe, tmp_path, img, max_file_size=len(data))[3] == 0
    assert _write(exe, tmp_path, img, max_file_size=len(data) - 1)[3] == 98       # TOO_LARGE_FILE


def test_a_palette_that_cannot_be_written_is_refused(exe, tmp_path):
    img = _image(5, 2, 4, 4, seed=9)
    r = X.restate(img)
    (tmp_path / "z.bin").write_bytes(zlib.compress(r["scanlines"], 9))
    (tmp_path / "empty.bin").write_bytes(b"")
    (tmp_path / "trns.bin").write_bytes(bytes(6))                       # more tRNS entries than palette entries
    (tmp_path / "plte.bin").write_bytes(r["plte"])
    for plte, trns in (("empty.bin", "-"), ("plte.bin", "trns.bin")):
        p = subprocess.run([exe, str(tmp_path / "o.png"), "4", "4", str(tmp_path / plte), str(tmp_path / trns) if trns != "-" else "-", str(tmp_path / "z.bin"), "-", "0"],
                           capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.split()[0] == "4", (p.stdout, p.stderr[-500:])     # INVALID_ARGUMENT

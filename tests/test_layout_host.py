"""The memory layouts of the host shim (pngloss_amd/csrc/pl_layout.h: the batch workspace of enqueue, the arena of a host window, the read side's
workspace and frame arena, the regrow rule, the colour type of an out-flags word) on the CPU through tests/c/layout_host.cpp.

For each layout: the invariants a GPU run would only show as a corrupted neighbour (every region on a 256-byte boundary, no two regions overlapping,
the total covering the last one) on a few hundred random batches with the shapes the code special-cases, and the PINNED VALUES: every offset equals
the arithmetic pl_host.hip did inline before the header existed, restated here in Python (py_* below, written from that code, not from the header).

What the layouts do not decide is not here: an image with a stream-only zlib stream has the same place in the window as any other image that
emits (whether its pixels come back is batch_host_one's predicate)."""
import struct

import numpy as np
import pytest

from tests import util as U

A = 256
NFILT, NSYM, ROWSTAT_WORDS = 5, 256, 5 * 256 + 8
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]     # x0, y0, dx, dy


def au(v, a=A):
    return (v + a - 1) // a * a


def check_regions(regions, total, what):
    """regions: (name, offset, bytes).  Aligned, disjoint, inside total; empty regions only have to be aligned."""
    for name, off, size in regions:
        assert off % A == 0 and off >= 0 and size >= 0, (what, name, off)
    live = sorted((off, off + size, name) for name, off, size in regions if size)
    for (a0, a1, an), (b0, b1, bn) in zip(live, live[1:]):
        assert a1 <= b0, (what, an, bn, a0, a1, b0)
    if live:
        assert live[-1][1] <= total, (what, live[-1], total)


# ------------------------------------------------------------------------------------------------ the batch workspace

WS_FIELDS = ["flags", "orig_hist", "orig_rank", "cand", "err0", "err1", "old_above", "final_hist", "result", "row_ids", "out_flags", "rowstat"]


def ws_sizes(w, h, rows):
    w = w or 1
    return {"flags": 4, "orig_hist": 4 * NFILT * NSYM, "orig_rank": 4 * NFILT * NSYM, "cand": 16 * NFILT * w, "err0": 8 * w, "err1": 8 * w, "old_above": 4 * w,
            "final_hist": 4 * NSYM, "result": 4 * 64, "row_ids": h or 1, "out_flags": 4, "rowstat": 4 * ROWSTAT_WORDS * (h or 1) if rows else 0}


def py_image_ws(w, h, rows):
    """image_ws() as pl_host.hip had it (the caller passed width ? width : 1)"""
    o, out = 0, {}
    for name in WS_FIELDS:
        size = ws_sizes(w, h, rows)[name]
        if name == "rowstat" and not rows:
            out[name] = 0
            continue
        out[name] = o
        o = au(o + size)
    out["total"] = o
    return out


def py_batch(ws, hs, rows, seg_list, n_wg, nsp, seeded, job_bytes, segjob_bytes):
    """the offset arithmetic of enqueue() as it stood"""
    n = len(ws)
    lib = U.layout_host_lib()
    total = au(job_bytes * (n or 1))
    offs = []
    for w, h in zip(ws, hs):
        offs.append(total)
        total += py_image_ws(w or 1, h, rows)["total"]
    seg_jobs = seg_params = sel = 0
    seg_offs = []
    if seg_list:
        seg_jobs = total; total += au(segjob_bytes * len(seg_list))
        seg_params = total; total += au(lib.layout_host_seg_params_bytes())
        sel = total; total += au(4 * (n_wg or 1))
        for i in seg_list:
            seg_offs.append(total)
            total += lib.layout_host_seg_total(ws[i] or 1, nsp, int(seeded))
    return offs, seg_jobs, seg_params, sel, seg_offs, total


def c_batch(ws, hs, rows, seg_list, n_wg, nsp, seeded, job_bytes, segjob_bytes):
    n, k = len(ws), len(seg_list)
    w, h, sl = np.array(ws, np.uint32), np.array(hs, np.uint32), np.array(seg_list, np.uint32)
    img, tables, seg = np.zeros((max(n, 1), 14), np.int64), np.zeros(4, np.int64), np.zeros((max(k, 1), 2), np.int64)
    U.layout_host_lib().layout_host_batch(w.ctypes.data, h.ctypes.data, n, int(rows), sl.ctypes.data, k, n_wg, nsp, int(seeded), job_bytes, segjob_bytes,
                                          img.ctypes.data, tables.ctypes.data, seg.ctypes.data)
    return img[:n], [int(x) for x in tables], seg[:k]


def random_batch(rng):
    n = int(rng.choice([0, 1, 2, 3, 8, int(rng.integers(0, 20))]))
    ws = [int(rng.choice([0, 1, 2, 63, 64, 65, 640, 1920, int(rng.integers(1, 5000))])) for _ in range(n)]
    hs = [int(rng.choice([0, 1, 2, 255, 256, 257, int(rng.integers(1, 3000))])) for _ in range(n)]
    on_seg = [i for i in range(n) if rng.random() < 0.5] if rng.random() < 0.7 else []
    seg_list = [int(i) for i in rng.permutation(on_seg)]
    return ws, hs, bool(rng.integers(0, 2)), seg_list, n - len(seg_list), int(rng.choice([16, 64, 256])), bool(rng.integers(0, 2)), int(rng.choice([8, 152, 160])), int(rng.choice([8, 232, 256]))


def test_batch_workspace_invariants_and_pinned_values():
    rng = np.random.default_rng(11)
    lib = U.layout_host_lib()
    cases = [random_batch(rng) for _ in range(300)]
    cases += [([], [], False, [], 0, 64, False, 152, 232), ([0], [0], True, [0], 0, 64, True, 152, 232), ([7, 0, 9], [0, 5, 3], True, [2, 0], 1, 256, False, 152, 232)]
    for case in cases:
        ws, hs, rows, seg_list, n_wg, nsp, seeded, job_bytes, segjob_bytes = case
        img, (seg_jobs, seg_params, sel, total), seg = c_batch(*case)
        want = py_batch(*case)
        assert ([int(r[0]) for r in img], seg_jobs, seg_params, sel, [int(s[0]) for s in seg], total) == want, case
        regions = [("jobs", 0, job_bytes * (len(ws) or 1))]
        for i, (w, h) in enumerate(zip(ws, hs)):
            pw = py_image_ws(w or 1, h, rows)
            assert [int(x) for x in img[i, 1:]] == [pw[f] for f in WS_FIELDS] + [pw["total"]], (case, i)
            sizes = ws_sizes(w, h, rows)
            regions += [("image %d %s" % (i, f), int(img[i, 0] + img[i, 1 + k]), sizes[f]) for k, f in enumerate(WS_FIELDS)]
            assert int(img[i, 13]) % A == 0
        if seg_list:
            regions += [("seg jobs", seg_jobs, segjob_bytes * len(seg_list)), ("seg params", seg_params, lib.layout_host_seg_params_bytes()), ("selection", sel, 4 * (n_wg or 1))]
            for k, i in enumerate(seg_list):
                assert int(seg[k, 1]) == lib.layout_host_seg_total(ws[i] or 1, nsp, int(seeded))
                regions.append(("seg image %d" % i, int(seg[k, 0]), int(seg[k, 1])))
        check_regions(regions, total, case)


def test_row_counter_bytes_are_the_rule_of_the_memory_check():
    """the strength-0 memory check of enqueue adds up align_up(4 * PL_ROWSTAT_WORDS * max(height, 1), 256) -- and image_ws takes exactly that for its counters"""
    lib = U.layout_host_lib()
    for h in [0, 1, 2, 3, 63, 64, 1080, 4096, 65535, 1 << 20]:
        assert lib.layout_host_rowstat_bytes(h) == au(4 * ROWSTAT_WORDS * (h or 1))
        img, (_, _, _, total), _ = c_batch([5], [h], True, [], 1, 64, False, 152, 232)
        assert int(img[0, 13]) - int(img[0, 12]) == lib.layout_host_rowstat_bytes(h)


# ------------------------------------------------------------------------------------------------ the arena of a host window

def py_window(ws, hs, filt, emit):
    """the offset arithmetic of batch_host_one() as it stood; per image (px, img, flt, span, ids, rows, pitch), then mirrored and total"""
    n, total = len(ws), 0
    img, flt = [0] * n, [0] * n
    for i in range(n):
        px = ws[i] * hs[i]
        img[i] = total; total = au(total + px * 4)
        flt[i] = total; total = au(total + (hs[i] if filt[i] else 0))
    mirrored, out = total, []
    for i in range(n):
        px = ws[i] * hs[i]
        want = bool(emit[i] and px)
        pitch = au(ws[i] * 4, 16) if want else 0
        ids = total; total = au(total + (hs[i] if want else 0))
        rows = total; total = au(total + pitch * (hs[i] if want else 0))
        span = flt[i] + hs[i] - img[i] if filt[i] else px * 4       # "the filter flags sit right behind the image: one copy takes both"
        out.append((px, img[i], flt[i], span, ids, rows, pitch))
    return out, mirrored, total


def c_window(ws, hs, filt, emit):
    n = len(ws)
    w, h, f, e = np.array(ws, np.uint32), np.array(hs, np.uint32), np.array(filt, np.uint8), np.array(emit, np.uint8)
    im, tot = np.zeros((max(n, 1), 7), np.int64), np.zeros(2, np.int64)
    U.layout_host_lib().layout_host_window(w.ctypes.data, h.ctypes.data, f.ctypes.data, e.ctypes.data, n, im.ctypes.data, tot.ctypes.data)
    return [tuple(int(x) for x in r) for r in im[:n]], int(tot[0]), int(tot[1])


def test_window_arena_invariants_and_pinned_values():
    rng = np.random.default_rng(12)
    cases = []
    for _ in range(300):
        n = int(rng.choice([0, 1, 2, 5, int(rng.integers(0, 30))]))
        ws = [int(rng.choice([0, 1, 3, 4, 5, 64, 1280, int(rng.integers(1, 3000))])) for _ in range(n)]
        hs = [int(rng.choice([0, 1, 2, 255, 256, 257, 720, int(rng.integers(1, 2000))])) for _ in range(n)]
        mode = int(rng.integers(0, 4))              # filters / emit for none, all, or some of the images
        filt = [mode == 1 or (mode >= 2 and rng.random() < 0.5) for _ in range(n)]
        mode = int(rng.integers(0, 4))
        emit = [mode == 1 or (mode >= 2 and rng.random() < 0.5) for _ in range(n)]
        cases.append((ws, hs, filt, emit))
    cases += [([], [], [], []), ([0, 5, 0], [7, 0, 0], [True, True, False], [True, True, True]), ([3], [2], [False], [True])]
    for ws, hs, filt, emit in cases:
        im, mirrored, total = c_window(ws, hs, filt, emit)
        assert (im, mirrored, total) == py_window(ws, hs, filt, emit), (ws, hs, filt, emit)
        assert mirrored <= total and mirrored % A == 0 and total % A == 0
        regions = []
        for i, (px, img, flt, span, ids, rows, pitch) in enumerate(im):
            assert px == ws[i] * hs[i]
            assert (pitch != 0) == bool(emit[i] and px) and pitch % 16 == 0 and (pitch == 0 or ws[i] * 4 <= pitch < ws[i] * 4 + 16)
            regions += [("image %d" % i, img, px * 4), ("flags %d" % i, flt, hs[i] if filt[i] else 0),
                        ("ids %d" % i, ids, hs[i] if pitch else 0), ("rows %d" % i, rows, pitch * hs[i] if pitch else 0)]
            # the one copy that brings the image back: from the image's first byte to the last of its pixels, or -- with flags, which are the very next
            # region -- to the last flag; it touches no other image and stays inside the mirrored prefix
            assert img + px * 4 <= flt and flt == au(img + px * 4)
            assert img + span == (flt + hs[i] if filt[i] else img + px * 4)
            assert img + span <= mirrored and (i + 1 == len(im) or img + span <= im[i + 1][1])
            assert img + px * 4 <= mirrored and flt + (hs[i] if filt[i] else 0) <= mirrored and ids >= mirrored and rows >= mirrored
        check_regions(regions, total, (ws, hs, filt, emit))


# ------------------------------------------------------------------------------------------------ the read side

def py_pass(p, w, h, ctype, depth):
    x0, y0, dx, dy = ADAM7[p]
    pw = (w - x0 + dx - 1) // dx if w > x0 else 0
    ph = (h - y0 + dy - 1) // dy if h > y0 else 0
    rb = (pw * CHANNELS[ctype] * depth + 7) // 8
    return x0, y0, dx, dy, pw, ph, rb, ph * (1 + rb) if pw and ph else 0


def py_read(files, frames, job_bytes, stream_bytes):
    """the offset arithmetic of png_decode_body() as it stood: data offsets relative to the region behind the tables, the tables' size added at the end;
    returns what its pointers were, as offsets into the workspace (or, for `out` with frames, the frame arena)"""
    n = len(files)
    total = ftotal = nprog = max_bands = 0
    raw_off, z_off, out_off, raw_bytes, jobs = [0] * n, [0] * n, [0] * n, [0] * n, []
    for i, (w, h, ct, d, il, zb) in enumerate(files):
        passes = [py_pass(p, w, h, ct, d) for p in range(7)]
        pass_off = [sum(s[7] for s in passes[:p]) for p in range(7)]
        rowbytes = (w * CHANNELS[ct] * d + 7) // 8
        raw_bytes[i] = sum(s[7] for s in passes) if il else h * (1 + rowbytes)
        raw_off[i] = total; total += au(raw_bytes[i])
        if zb >= 0:
            z_off[i] = total; total += au(zb + 16)
        out_bytes = au(w * h * 4)
        if frames:
            out_off[i] = ftotal; ftotal += out_bytes
        else:
            out_off[i] = total; total += out_bytes
        for p in range(7 if il else 1):
            if il:
                x0, y0, dx, dy, jw, jh, jrb, nbytes = passes[p]
                if not nbytes:
                    continue
            else:
                x0, y0, dx, dy, jw, jh, jrb = 0, 0, 1, 1, w, h, rowbytes
            nbands, lastpitch = (jh + 63) // 64, au(jrb)
            max_bands = max(max_bands, nbands)
            jobs.append(dict(file=i, raw=pass_off[p] if il else 0, last=total, prog=nprog, geo=[x0, y0, dx, dy, w, nbands, lastpitch, jw, jh, jrb]))
            total += lastpitch * nbands
            nprog += nbands
    m = len(jobs)
    jobs_bytes, st_bytes, prog_bytes, zjobs_bytes = au(job_bytes * m), au(4 * n), au(4 * nprog), au(stream_bytes * n)
    head = jobs_bytes + 2 * st_bytes + prog_bytes + zjobs_bytes
    total += head
    fb = 0 if frames else head
    tables = [jobs_bytes, jobs_bytes + st_bytes, jobs_bytes + 2 * st_bytes, jobs_bytes + 2 * st_bytes + prog_bytes, 2 * st_bytes + prog_bytes, max_bands, nprog, total, ftotal]
    fl = [[raw_bytes[i], head + raw_off[i], head + z_off[i] if files[i][5] >= 0 else 0, fb + out_off[i]] for i in range(n)]
    jl = [[j["file"], head + raw_off[j["file"]] + j["raw"], head + j["last"], j["prog"]] + j["geo"] for j in jobs]
    return tables, fl, jl, dict(jobs_bytes=job_bytes * m, st=4 * n, prog=4 * nprog, zjobs=stream_bytes * n)


def c_read(files, frames, job_bytes, stream_bytes):
    n = len(files)
    inp = np.array(files, np.int64).reshape(n, 6) if n else np.zeros((1, 6), np.int64)
    head, fl, jl = np.zeros(9, np.int64), np.zeros((max(n, 1), 4), np.int64), np.zeros((max(7 * n, 1), 14), np.int64)
    m = U.layout_host_lib().layout_host_read(inp.ctypes.data, n, int(frames), job_bytes, stream_bytes, head.ctypes.data, fl.ctypes.data, jl.ctypes.data)
    return [int(x) for x in head], [[int(x) for x in r] for r in fl[:n]], [[int(x) for x in r] for r in jl[:m]]


FORMATS = [(6, 8), (6, 16), (2, 8), (2, 16), (0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16)]


def random_files(rng, zs):
    n = int(rng.choice([0, 1, 2, 7, int(rng.integers(0, 16))]))
    out = []
    for _ in range(n):
        ct, d = FORMATS[int(rng.integers(0, len(FORMATS)))]
        small = rng.random() < 0.6              # (interlaced files up to 8 x 8 have empty passes)
        w = int(rng.integers(1, 9)) if small else int(rng.choice([63, 64, 65, 129, int(rng.integers(9, 2500))]))
        h = int(rng.integers(1, 9)) if small else int(rng.choice([63, 64, 65, 129, int(rng.integers(9, 1500))]))
        out.append((w, h, ct, d, int(rng.integers(0, 2)), int(rng.choice([6, 7, 240, 241, int(rng.integers(6, 100000))])) if zs else -1))
    return out


@pytest.mark.parametrize("frames", [False, True])
@pytest.mark.parametrize("zs", [False, True])
def test_read_side_invariants_and_pinned_values(frames, zs):
    rng = np.random.default_rng(13 + 2 * frames + zs)
    cases = [random_files(rng, zs) for _ in range(200)]
    cases.append([(w, h, 6, 8, 1, 64 if zs else -1) for w in range(1, 9) for h in range(1, 9)])
    assert U.layout_host_lib().layout_host_band_rows() == 64
    for files in cases:
        job_bytes, stream_bytes = int(rng.choice([8, 1112, 1120])), int(rng.choice([8, 32, 40]))
        head, fl, jl = c_read(files, frames, job_bytes, stream_bytes)
        want_head, want_fl, want_jl, tbl = py_read(files, frames, job_bytes, stream_bytes)
        assert (head, fl, jl) == (want_head, want_fl, want_jl), files
        status, zstatus, prog, zjobs, zeroed, max_bands, nprog, total, ftotal = head
        assert zeroed == zjobs - status                 # one memset: both status arrays and the progress words
        regions = [("jobs", 0, tbl["jobs_bytes"]), ("status", status, tbl["st"]), ("zstatus", zstatus, tbl["st"]), ("progress", prog, tbl["prog"]), ("streams", zjobs, tbl["zjobs"])]
        fregions = []
        for i, (w, h, ct, d, il, zb) in enumerate(files):
            raw_bytes, raw, z, out = fl[i]
            regions.append(("raw %d" % i, raw, raw_bytes))
            if zb >= 0:
                regions.append(("z %d" % i, z, zb + 16))
            (fregions if frames else regions).append(("rgba %d" % i, out, w * h * 4))
        covered = {}
        for k, (f, raw, last, pr, ox, oy, sx, sy, pitch, nbands, lastpitch, jw, jh, jrb) in enumerate(jl):
            regions.append(("last rows %d" % k, last, lastpitch * nbands))
            assert lastpitch % A == 0 and lastpitch >= jrb and nbands == (jh + 63) // 64 and nbands <= max_bands and pitch == files[f][0]
            assert fl[f][1] <= raw and raw + jh * (1 + jrb) <= fl[f][1] + fl[f][0]          # the job's scanlines lie inside its file's
            covered[f] = covered.get(f, 0) + jh * (1 + jrb)
            assert pr == sum(j[9] for j in jl[:k])
        assert all(covered.get(i, 0) == fl[i][0] for i in range(len(files)))                # ... and the jobs of a file take all of them
        assert nprog == sum(j[9] for j in jl) and max_bands == max([j[9] for j in jl] + [0])
        check_regions(regions, total, files)
        check_regions(fregions, ftotal, files)
        assert ftotal == 0 or frames


def adam7_fixture_shapes():
    """(width, height, bit depth, colour type, interlace) from the IHDR of every file of tests/golden/png_read_adam7_cases.npz"""
    g = U.load_npz("png_read_adam7_cases.npz")
    shapes = set()
    for k in g.files:
        if k.endswith("/png"):
            w, h, depth, ct, _, _, il = struct.unpack(">IIBBBBB", g[k].tobytes()[16:29])
            shapes.add((w, h, depth, ct, il))
    return sorted(shapes)


def test_adam7_jobs_of_the_fixtures_shapes_are_the_passes():
    """one job per non-empty pass, with the geometry pr_adam7_pass gives (and the specification's table, stated in Python)"""
    lib = U.layout_host_lib()
    shapes = adam7_fixture_shapes()
    assert len(shapes) >= 50 and any(il for *_, il in shapes)
    ps = np.zeros(8, np.int64)
    for w, h, depth, ct, il in shapes:
        head, fl, jl = c_read([(w, h, ct, depth, il, -1)], False, 1112, 32)
        want, off = [], 0
        for p in range(7 if il else 1):
            if il:
                lib.layout_host_adam7_pass(p, w, h, ct, depth, ps.ctypes.data)
                assert tuple(int(x) for x in ps) == py_pass(p, w, h, ct, depth)
                x0, y0, dx, dy, pw, ph, rb, nbytes = (int(x) for x in ps)
            else:
                x0, y0, dx, dy, pw, ph, rb = 0, 0, 1, 1, w, h, (w * CHANNELS[ct] * depth + 7) // 8
                nbytes = ph * (1 + rb)
            if nbytes:
                want.append([fl[0][1] + off, x0, y0, dx, dy, w, (ph + 63) // 64, au(rb), pw, ph, rb])
            off += nbytes
        assert [[j[1]] + j[4:] for j in jl] == want, (w, h, depth, ct, il)
        assert off == fl[0][0]


# ------------------------------------------------------------------------------------------------ the small pure pieces

def test_grow_bytes():
    lib = U.layout_host_lib()
    rng = np.random.default_rng(14)
    for divisor in (4, 8):
        for _ in range(2000):
            need = int(rng.choice([0, 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, int(rng.integers(0, 1 << 36))]))
            have = int(rng.choice([0, need, max(need - 1, 0), need + 1, int(rng.integers(0, 1 << 36))]))
            got = lib.layout_host_grow(need, have, divisor)
            if need <= have:
                assert got == 0                                 # no growth
            else:
                assert got == au(need + need // divisor, 1 << 20) and got >= need and got % (1 << 20) == 0


def test_colour_type_and_bytes_per_pixel_of_the_out_flags():
    lib = U.layout_host_lib()
    GRAY, OPAQUE = 1, 2
    want = {0: (6, 4), OPAQUE: (2, 3), GRAY: (4, 2), GRAY | OPAQUE: (0, 1)}
    for flags, (ct, bpp) in want.items():
        for junk in (0, 4, 0xFFFFFFFC):             # (only the two class bits count)
            assert (lib.layout_host_color_type(flags | junk), lib.layout_host_emit_bpp(flags | junk)) == (ct, bpp)


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_pack_and_unpack_rows(bpp):
    """a packed pixel's channel c is byte c of its slots word, the bytes beyond bpp are 0; unpack is the inverse and ignores them"""
    lib = U.layout_host_lib()
    rng = np.random.default_rng(bpp)
    for width in (1, 2, 17, 256):
        packed = rng.integers(0, 256, (width, bpp), dtype=np.uint8)
        slots = np.full(width, 0xDEADBEEF, np.uint32)
        lib.layout_host_pack(slots.ctypes.data, packed.ctypes.data, width, bpp)
        want = np.zeros((width, 4), np.uint8)
        want[:, :bpp] = packed
        assert np.array_equal(slots.view(np.uint8).reshape(width, 4), want)
        dirty = slots | (np.uint32(0xFFFFFFFF) << np.uint32(8 * bpp) if bpp < 4 else np.uint32(0))
        back = np.zeros((width, bpp), np.uint8)
        lib.layout_host_unpack(back.ctypes.data, np.ascontiguousarray(dirty, np.uint32).ctypes.data, width, bpp)
        assert np.array_equal(back, packed)

/*
 * pl_layout.h -- every carve-up of a buffer the host shim makes, as pure functions from sizes to offsets: the batch workspace of enqueue(), the
 * arena of a host window (batch_host_one), the keep arena of the distortion measurement, the tables of the SSIM measurement, the index workspace of the option "indexed" and the packed rows of "index_depth" behind it, the quantiser's workspace and the job table and error lines of its dither pass, the read side's workspace and frame arena
 * (png_decode_body), and the size a buffer is regrown to.
 * Internal.
 *
 * Plain C++17 without HIP, like pl_plan.h: the pl_host*.hip files turn the offsets into pointers, copies and launches, and tests/c/layout_host.cpp compiles
 * the same header with g++ so that the CPU suite proves alignment, disjointness and the pinned values (tests/test_layout_host.py).  The job
 * structs live in headers that include the HIP runtime, so their sizes come in as arguments; what the header states about the device side
 * itself (PLL_*) is pinned by static_asserts in pl_host_ctx.h.
 */
#ifndef PL_LAYOUT_H
#define PL_LAYOUT_H

#include "pl_plan.h"
#include "pl_pngread_core.h"
#include "pl_index_core.h"
#include "pl_quant_core.h"
#include "pl_dither_core.h"

#include <cstdint>
#include <cstring>
#include <vector>

constexpr size_t PLL_ALIGN = 256;                      /* every region of every layout starts on a multiple of it */
constexpr size_t PLL_NFILT = 5, PLL_NSYM = 256;        /* PL_NFILT, PL_NSYM */
constexpr size_t PLL_ROWSTAT_WORDS = PLL_NFILT * PLL_NSYM + 8;   /* PL_ROWSTAT_WORDS */
constexpr size_t PLL_UINT4 = 16, PLL_UINT2 = 8;        /* sizeof(uint4), sizeof(uint2) */
constexpr uint32_t PLL_FLAG_GRAY = 1u, PLL_FLAG_OPAQUE = 2u;     /* PL_FLAG_GRAY, PL_FLAG_OPAQUE */

inline size_t pl_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* ---- regrow on demand: 0 when `have` bytes are enough for `need`, else the size to allocate -- need plus need / divisor of slack, in whole MiB ---- */
inline size_t pl_grow_bytes(size_t need, size_t have, size_t divisor)
{
    return need <= have ? 0 : pl_align_up(need + need / divisor, (size_t)1 << 20);
}

/* ---- the PNG colour type and the bytes per pixel of an optimised image, from its out-flags word (PL_FLAG_*, PlJob::out_flags) ---- */
inline int pl_color_type_of(uint32_t flags) { return (flags & PLL_FLAG_GRAY) ? ((flags & PLL_FLAG_OPAQUE) ? 0 : 4) : ((flags & PLL_FLAG_OPAQUE) ? 2 : 6); }
inline uint32_t pl_emit_bpp_of(uint32_t flags) { return (flags & PLL_FLAG_GRAY) ? ((flags & PLL_FLAG_OPAQUE) ? 1u : 2u) : ((flags & PLL_FLAG_OPAQUE) ? 3u : 4u); }

/* ---- a row of packed bpp-byte pixels to and from "slots" words (pl_device.h: channel c in byte c) ---- */
inline void pl_pack_row(uint32_t *slots, const unsigned char *packed, uint32_t width, uint32_t bpp)
{
    if (bpp == 4) { std::memcpy(slots, packed, (size_t)width * 4); return; }
    for (uint32_t x = 0; x < width; x++) {
        uint32_t w = 0;
        for (uint32_t c = 0; c < bpp; c++) w |= (uint32_t)packed[(size_t)x * bpp + c] << (8 * c);
        slots[x] = w;
    }
}
inline void pl_unpack_row(unsigned char *packed, const uint32_t *slots, uint32_t width, uint32_t bpp)
{
    if (bpp == 4) { std::memcpy(packed, slots, (size_t)width * 4); return; }
    for (uint32_t x = 0; x < width; x++)
        for (uint32_t c = 0; c < bpp; c++) packed[(size_t)x * bpp + c] = (unsigned char)(slots[x] >> (8 * c));
}

/* ================================================================================================ the batch workspace (enqueue) */

struct WsLayout {
    size_t flags, orig_hist, orig_rank, cand, err0, err1, old_above, final_hist, result, row_ids, out_flags, rowstat, total;
};

/* the row-statistics engine's counters of one image (strength 0: pl_rows.hip): PLL_ROWSTAT_WORDS per row -- also what enqueue's memory check adds up */
inline size_t pl_rowstat_bytes(uint32_t height) { return pl_align_up(sizeof(uint32_t) * PLL_ROWSTAT_WORDS * (size_t)(height ? height : 1), PLL_ALIGN); }

/* per-image workspace: everything the engine keeps outside the image itself (width: at least 1) */
inline WsLayout image_ws(uint32_t width, uint32_t height, bool rows_engine)
{
    WsLayout l{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = pl_align_up(o + bytes, PLL_ALIGN); return at; };
    l.flags = take(sizeof(uint32_t));
    l.orig_hist = take(sizeof(uint32_t) * PLL_NFILT * PLL_NSYM);
    l.orig_rank = take(sizeof(uint32_t) * PLL_NFILT * PLL_NSYM);
    l.cand = take(PLL_UINT4 * PLL_NFILT * (size_t)width);
    l.err0 = take(PLL_UINT2 * (size_t)width);
    l.err1 = take(PLL_UINT2 * (size_t)width);
    l.old_above = take(sizeof(uint32_t) * (size_t)width);
    l.final_hist = take(sizeof(uint32_t) * PLL_NSYM);
    l.result = take(sizeof(int32_t) * 64);
    l.row_ids = take(height ? height : 1);
    l.out_flags = take(sizeof(uint32_t));
    l.rowstat = rows_engine ? take(pl_rowstat_bytes(height)) : 0;
    l.total = o;
    return l;
}

/* The PlJob table at 0, then one image_ws() block per image; for a batch with images on the segment engine the SegJob table, SegParams, the
 * selection list of the other engine's images and one pl_seg_layout() block per entry of seg_list follow. */
struct PlBatchLayout {
    std::vector<size_t> image;          /* [n] base of the image's block */
    std::vector<WsLayout> ws;           /* [n] offsets inside it */
    size_t seg_jobs = 0, seg_params = 0, sel = 0;
    std::vector<size_t> seg_image;      /* [seg_list.size()] base of the segment engine's block of image seg_list[k] */
    std::vector<PlSegLayout> seg;       /* ... and the offsets inside it */
    size_t total = 0;
};

/* seg_list, n_wg, nsp, seeded: PlPlan::seg_list, ::wg_list.size(), ::params.nsp and ::params.seeded; job_bytes, segjob_bytes: sizeof(PlJob), sizeof(SegJob) */
inline PlBatchLayout pl_batch_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool use_rows, const std::vector<uint32_t> &seg_list,
                                     size_t n_wg, uint32_t nsp, bool seeded, size_t job_bytes, size_t segjob_bytes)
{
    PlBatchLayout b;
    const size_t n = width.size();
    auto take = [&](size_t bytes) { size_t at = b.total; b.total += pl_align_up(bytes, PLL_ALIGN); return at; };
    take(job_bytes * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        b.ws.push_back(image_ws(width[i] ? width[i] : 1, height[i], use_rows));
        b.image.push_back(take(b.ws[i].total));
    }
    if (seg_list.empty()) return b;
    b.seg_jobs = take(segjob_bytes * seg_list.size());
    b.seg_params = take(sizeof(SegParams));
    b.sel = take(sizeof(uint32_t) * (n_wg ? n_wg : 1));
    for (uint32_t i : seg_list) {
        b.seg.push_back(pl_seg_layout(width[i] ? width[i] : 1, nsp, seeded));
        b.seg_image.push_back(take(b.seg.back().total));
    }
    return b;
}

/* ================================================================================================ the arena of a host window (batch_host_one) */

/* One device arena for the whole window: first [image | filter flags] of every image -- the part that has a pinned mirror of the same layout on
 * the host --, behind them [emitted ids | emitted rows] of every image that wants them (those come back straight into the caller's memory). */
struct PlWindowIn { uint32_t width, height; bool filters, emit; };      /* filters: the caller wants the filter flags; emit: ... scanlines or a zlib stream */
struct PlWindowImage {
    size_t px;              /* width * height */
    size_t img, flt;        /* px * 4 bytes; height bytes (none without `filters`) */
    size_t span;            /* the ONE copy that brings an image back: from `img`, its pixels and -- they sit right behind the image, only padding between -- its filter flags */
    size_t ids, rows;       /* height bytes; height * pitch bytes (none when pitch is 0) */
    uint32_t pitch;         /* of the emitted rows; 0: nothing is emitted for this image (not wanted, or no pixels) */
};
struct PlWindowLayout {
    std::vector<PlWindowImage> im;
    size_t mirrored = 0, total = 0;     /* [0, mirrored) has the pinned twin */
};

inline PlWindowLayout pl_window_layout(const std::vector<PlWindowIn> &in)
{
    PlWindowLayout w;
    w.im.resize(in.size());
    auto take = [&](size_t bytes) { size_t at = w.total; w.total = pl_align_up(w.total + bytes, PLL_ALIGN); return at; };
    for (size_t i = 0; i < in.size(); i++) {
        PlWindowImage &m = w.im[i];
        m.px = (size_t)in[i].width * in[i].height;
        m.img = take(m.px * 4);
        m.flt = take(in[i].filters ? in[i].height : 0);
        m.span = in[i].filters ? m.flt + in[i].height - m.img : m.px * 4;
    }
    w.mirrored = w.total;
    for (size_t i = 0; i < in.size(); i++) {
        PlWindowImage &m = w.im[i];
        const bool want = in[i].emit && m.px;
        m.pitch = want ? (uint32_t)pl_align_up((size_t)in[i].width * 4, 16) : 0;
        m.ids = take(want ? in[i].height : 0);
        m.rows = take((size_t)m.pitch * (want ? in[i].height : 0));
    }
    return w;
}

/* ================================================================================================ the keep arena (option "distortion": enqueue, compare_batch) */

/* The PlDistortJob table at 0, then one record per image, then -- with `originals` -- room for the original RGBA8 of every image (pl_keep fills it,
 * pl_distort reads it).  pngloss_hip_compare_batch measures two images of the caller's and keeps nothing: tables only. */
struct PlKeepLayout {
    size_t jobs = 0, records = 0;
    std::vector<size_t> image;          /* [n] the image's original: width * height * 4 bytes (all 0 without `originals`) */
    size_t total = 0;
};

/* job_bytes, record_bytes: sizeof(PlDistortJob), sizeof(PlDistortRecord) */
inline PlKeepLayout pl_keep_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool originals, size_t job_bytes, size_t record_bytes)
{
    PlKeepLayout k;
    const size_t n = width.size();
    auto take = [&](size_t bytes) { size_t at = k.total; k.total = pl_align_up(k.total + bytes, PLL_ALIGN); return at; };
    k.jobs = take(job_bytes * (n ? n : 1));
    k.records = take(record_bytes * (n ? n : 1));
    k.image.assign(n, 0);
    if (originals)
        for (size_t i = 0; i < n; i++) k.image[i] = take((size_t)width[i] * height[i] * 4);
    return k;
}

/* ================================================================================================ the SSIM tables (option "ssim": enqueue, compare_batch_ssim) */

/* The PlSsimJob table at 0, then one record per image: a small buffer of its own.  The originals the jobs point at are the keep arena's, which the
 * options "distortion" and "ssim" share (pngloss_hip_compare_batch_ssim measures two images of the caller's). */
struct PlSsimLayout { size_t jobs = 0, records = 0, total = 0; };

/* job_bytes, record_bytes: sizeof(PlSsimJob), sizeof(PlSsimRecord) */
inline PlSsimLayout pl_ssim_layout(size_t n, size_t job_bytes, size_t record_bytes)
{
    PlSsimLayout l;
    l.jobs = 0;
    l.records = pl_align_up(job_bytes * (n ? n : 1), PLL_ALIGN);
    l.total = l.records + pl_align_up(record_bytes * (n ? n : 1), PLL_ALIGN);
    return l;
}

/* ================================================================================================ the size measurement (pl_deflate_measure) */

/* One record per image, as dfl_sizes (pl_deflate.hip) leaves it on the device and one copy brings it to the host: what the image's zlib stream
 * would be, had the deflate written it.  The device side's twin is dfl_size_record (pl_deflate_core.h); pl_deflate.hip pins the two together. */
struct PlSizeRecord {
    uint64_t bytes;         /* the complete stream, 78 DA ... Adler-32; 0 for an image without pixels (it gets no stream) */
    uint32_t adler;         /* Adler-32 of the scanlines */
    uint32_t kinds[3];      /* deflate blocks stored / fixed / dynamic */
};
constexpr size_t PLL_SIZE_RECORD = 24;                 /* sizeof(PlSizeRecord), sizeof(dfl_size_record) */
static_assert(sizeof(PlSizeRecord) == PLL_SIZE_RECORD, "PlSizeRecord has no padding");

/* ================================================================================================ the index workspace (option "indexed": window_deflate) */

/* The PlIndexJob table at 0; the counters and the palette records of all images back to back (`zeroed` bytes from `counts`: one memset to 0); the
 * tables of all images back to back (`tables_bytes` from `tables`: one memset to 0xFF, PLI_EMPTY in every slot); then per image with pixels its
 * filter type bytes and its index rows, as the deflate stage reads scanlines: rows `pitch` bytes apart, the pitch a multiple of 16 as the emit
 * stage's (pl_window_layout).  Every image gets its rows, eligible or not: which ones are is known only after the batch has run, and a buffer that
 * cannot be had has to fail the call before anything is enqueued. */
struct PlIndexImage { size_t table, ids, rows; uint32_t pitch; };
struct PlIndexLayout {
    size_t jobs = 0, counts = 0, records = 0, zeroed = 0, tables = 0, tables_bytes = 0, total = 0;
    std::vector<PlIndexImage> im;
};

/* job_bytes, record_bytes: sizeof(PlIndexJob), sizeof(PliRecord) */
inline PlIndexLayout pl_index_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, size_t job_bytes, size_t record_bytes)
{
    PlIndexLayout l;
    const size_t n = width.size(), n1 = n ? n : 1;
    auto take = [&](size_t bytes) { size_t at = l.total; l.total = pl_align_up(l.total + bytes, PLL_ALIGN); return at; };
    l.im.resize(n);
    l.jobs = take(job_bytes * n1);
    l.counts = take(sizeof(uint32_t) * n1);
    l.records = take(record_bytes * n1);
    l.zeroed = l.total - l.counts;
    l.tables_bytes = sizeof(uint64_t) * PLI_SLOTS * n1;
    l.tables = take(l.tables_bytes);
    for (size_t i = 0; i < n; i++) {
        PlIndexImage &m = l.im[i];
        const bool px = width[i] && height[i];
        m.table = l.tables + sizeof(uint64_t) * PLI_SLOTS * i;
        m.pitch = px ? (uint32_t)pl_align_up(width[i], 16) : 0;
        m.ids = take(px ? height[i] : 0);
        m.rows = take((size_t)m.pitch * (px ? height[i] : 0));
    }
    return l;
}

/* ================================================================================================ the packed index rows (option "index_depth": window_index) */

/* Behind the index workspace, from `base` (pl_index_layout's total) on: the PlPackJob table, then per image with pixels the filter type bytes and
 * the rows of its packed scanlines.  The depth of an image is known only after the batch has run, so the pitch is the one the widest packed depth
 * needs -- ceil(width * 4 / 8) bytes, a multiple of 16 as the other scanline pitches -- and the rows of a shallower depth lie the same distance
 * apart.  Every image gets its rows, for the reason every image gets its index rows. */
struct PlPackImage { size_t ids, rows; uint32_t pitch; };
struct PlPackLayout {
    size_t jobs = 0, total = 0;
    std::vector<PlPackImage> im;
};

/* job_bytes: sizeof(PlPackJob) */
inline PlPackLayout pl_index_pack_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, size_t base, size_t job_bytes)
{
    PlPackLayout l;
    const size_t n = width.size(), n1 = n ? n : 1;
    l.total = pl_align_up(base, PLL_ALIGN);
    auto take = [&](size_t bytes) { size_t at = l.total; l.total = pl_align_up(l.total + bytes, PLL_ALIGN); return at; };
    l.im.resize(n);
    l.jobs = take(job_bytes * n1);
    for (size_t i = 0; i < n; i++) {
        PlPackImage &m = l.im[i];
        const bool px = width[i] && height[i];
        m.pitch = px ? (uint32_t)pl_align_up(((size_t)width[i] + 1) / 2, 16) : 0;
        m.ids = take(px ? height[i] : 0);
        m.rows = take((size_t)m.pitch * (px ? height[i] : 0));
    }
    return l;
}

/* ================================================================================================ the quantiser's workspace (pngloss_hip_quantize_batch) */

/* The tables in front: the PlIndexJob, PlQuantJob and PlDistortJob tables; then what one memset zeroes (`zeroed` bytes from `counts`): the colour
 * counters, the palette records (PliRecord), the distortion records and the accumulators (PLQ_MAX_COLORS * PLQ_CELLS 64-bit cells per image); the
 * colour tables of pl_index_count (`tables_bytes` from `tables`: one memset to 0xFF); the histograms (`hists_bytes` from `hists`: one memset to 0,
 * 256 KiB per image) and the palettes (PLQ_MAX_COLORS words per image).  Behind them per image with pixels its quantised pixels (`out`, beside the
 * input: the distortion record is taken between the two before the copy back in place) and -- with `inputs`, the host form -- the input itself.
 * Every image gets its `out`, exact or not: which ones are is known only after the first synchronisation, and a buffer that cannot be had has to
 * fail the call before anything is enqueued. */
struct PlQuantImage { size_t table, hist, pal, acc, out, in; };
struct PlQuantLayout {
    size_t index_jobs = 0, quant_jobs = 0, distort_jobs = 0;
    size_t counts = 0, records = 0, distort_records = 0, accs = 0, zeroed = 0;
    size_t tables = 0, tables_bytes = 0, hists = 0, hists_bytes = 0, pals = 0, total = 0;
    std::vector<PlQuantImage> im;
};
constexpr size_t PLL_QUANT_ACC = sizeof(uint64_t) * PLQ_MAX_COLORS * PLQ_CELLS, PLL_QUANT_HIST = sizeof(uint32_t) * PLQ_BINS, PLL_QUANT_PAL = sizeof(uint32_t) * PLQ_MAX_COLORS;

/* index_job_bytes, quant_job_bytes, distort_job_bytes, record_bytes, distort_record_bytes: sizeof(PlIndexJob), sizeof(PlQuantJob), sizeof(PlDistortJob),
 * sizeof(PliRecord), sizeof(PlDistortRecord) */
inline PlQuantLayout pl_quant_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs, size_t index_job_bytes,
                                     size_t quant_job_bytes, size_t distort_job_bytes, size_t record_bytes, size_t distort_record_bytes)
{
    PlQuantLayout l;
    const size_t n = width.size(), n1 = n ? n : 1;
    auto take = [&](size_t bytes) { size_t at = l.total; l.total = pl_align_up(l.total + bytes, PLL_ALIGN); return at; };
    l.im.resize(n);
    l.index_jobs = take(index_job_bytes * n1);
    l.quant_jobs = take(quant_job_bytes * n1);
    l.distort_jobs = take(distort_job_bytes * n1);
    l.counts = take(sizeof(uint32_t) * n1);
    l.records = take(record_bytes * n1);
    l.distort_records = take(distort_record_bytes * n1);
    l.accs = take(PLL_QUANT_ACC * n1);
    l.zeroed = l.total - l.counts;
    l.tables_bytes = sizeof(uint64_t) * PLI_SLOTS * n1;
    l.tables = take(l.tables_bytes);
    l.hists_bytes = PLL_QUANT_HIST * n1;
    l.hists = take(l.hists_bytes);
    l.pals = take(PLL_QUANT_PAL * n1);
    for (size_t i = 0; i < n; i++) {
        PlQuantImage &m = l.im[i];
        const size_t bytes = (size_t)width[i] * height[i] * 4;
        m.table = l.tables + sizeof(uint64_t) * PLI_SLOTS * i;
        m.hist = l.hists + PLL_QUANT_HIST * i;
        m.pal = l.pals + PLL_QUANT_PAL * i;
        m.acc = l.accs + PLL_QUANT_ACC * i;
        m.out = take(bytes);
        m.in = take(inputs ? bytes : 0);
    }
    return l;
}

/* ================================================================================================ the dither pass of the quantiser (pngloss_hip_quantize_batch2) */

/* Behind the quantiser's workspace, from `base` (pl_quant_layout's total) on: the PlDitherJob table, then per image its error line -- one PlfErr per
 * column, what the last row of a band of pl_dither leaves for the band below.  `lines_bytes` from `lines` holds them all.  Every image gets its
 * line, working image or not, for the reason every image gets its `out`. */
struct PlDitherLayout {
    size_t jobs = 0, lines = 0, lines_bytes = 0, total = 0;
    std::vector<size_t> line;
};

/* job_bytes: sizeof(PlDitherJob) */
inline PlDitherLayout pl_dither_layout(const std::vector<uint32_t> &width, size_t base, size_t job_bytes)
{
    PlDitherLayout l;
    const size_t n = width.size(), n1 = n ? n : 1;
    l.total = pl_align_up(base, PLL_ALIGN);
    auto take = [&](size_t bytes) { size_t at = l.total; l.total = pl_align_up(l.total + bytes, PLL_ALIGN); return at; };
    l.jobs = take(job_bytes * n1);
    l.lines = l.total;
    l.line.resize(n);
    for (size_t i = 0; i < n; i++) l.line[i] = take(PLF_ERR_BYTES * width[i]);
    l.lines_bytes = l.total - l.lines;
    return l;
}

/* ================================================================================================ the read side (png_decode_body) */

constexpr uint64_t PL_READ_NO_STREAM = ~(uint64_t)0;
struct PlReadIn { uint32_t width, height; int color_type, bit_depth, interlace; uint64_t zbytes; };   /* a valid PNG format (pr_format); zbytes: PL_READ_NO_STREAM, or the zlib stream to inflate on the device */
struct PlReadFile {
    uint64_t raw_bytes;     /* the inflated scanlines */
    size_t raw, z, out;     /* raw_bytes; zbytes + 16 (with a stream); width * height * 4: the RGBA8 -- in the workspace, or with `frames` in the frame arena */
};
/* one job per non-interlaced file, one per non-empty Adam7 pass of an interlaced one (pl_pngread.h: PrJob) */
struct PlReadJob {
    size_t file;
    size_t raw;             /* workspace: the job's part of the file's scanlines */
    size_t last;            /* workspace: per band of PR_ROWS rows its last row, `lastpitch` bytes each (for the band below) */
    size_t prog;            /* index of the job's first progress word: one per band */
    uint32_t ox, oy, sx, sy, pitch, nbands, lastpitch;      /* PrJob's */
    uint32_t width, height, rowbytes;                       /* PrJob::F's: the file's, or the pass's own */
};
/* Workspace: the tables in front -- jobs at 0, then the status words of the decode and of the inflate and the progress words (`zeroed` bytes from
 * `status`: one memset), then the inflate's streams --, behind them per file [scanlines | zlib stream | RGBA8 unless `frames` | last rows of its jobs]. */
struct PlReadLayout {
    size_t status = 0, zstatus = 0, prog = 0, zjobs = 0, zeroed = 0;
    bool frames = false;
    std::vector<PlReadFile> file;
    std::vector<PlReadJob> job;
    uint32_t max_bands = 0;
    size_t nprog = 0, total = 0, ftotal = 0;        /* progress words; bytes of the workspace and of the frame arena */
};

/* frames: the decoded images stay on the device, in the frame arena; job_bytes, stream_bytes: sizeof(PrJob), sizeof(PliStream) */
inline PlReadLayout pl_read_layout(const std::vector<PlReadIn> &in, bool frames, size_t job_bytes, size_t stream_bytes)
{
    PlReadLayout r;
    r.frames = frames;
    const size_t n = in.size();
    r.file.resize(n);
    /* the data first, relative to its start: how many jobs and progress words there are decides the size of the tables in front of it */
    size_t data = 0;
    auto take = [&](size_t bytes) { size_t at = data; data += pl_align_up(bytes, PLL_ALIGN); return at; };
    for (size_t i = 0; i < n; i++) {
        const PlReadIn &f = in[i];
        PlReadFile &o = r.file[i];
        uint64_t pass_off[PR_ADAM7_PASSES] = {};
        o.raw_bytes = f.interlace ? pr_adam7_bytes(f.width, f.height, f.color_type, f.bit_depth, pass_off) : pr_scanline_bytes(f.width, f.height, f.color_type, f.bit_depth, 0);
        o.raw = take(o.raw_bytes);
        o.z = f.zbytes != PL_READ_NO_STREAM ? take(f.zbytes + 16) : 0;
        const size_t out_bytes = pl_align_up((size_t)f.width * f.height * 4, PLL_ALIGN);
        if (frames) { o.out = r.ftotal; r.ftotal += out_bytes; } else o.out = take(out_bytes);
        for (int p = 0; p < (f.interlace ? PR_ADAM7_PASSES : 1); p++) {
            PlReadJob j{};
            j.file = i;
            if (f.interlace) {
                const PrPass ps = pr_adam7_pass(p, f.width, f.height, f.color_type, f.bit_depth);
                if (!ps.bytes) continue;                                          /* an empty pass has no bytes in the stream */
                j.width = ps.width; j.height = ps.height; j.rowbytes = ps.rowbytes;
                j.ox = ps.x0; j.oy = ps.y0; j.sx = ps.dx; j.sy = ps.dy;
            } else {
                j.width = f.width; j.height = f.height; j.rowbytes = pr_rowbytes(f.width, f.color_type, f.bit_depth);
                j.ox = 0; j.oy = 0; j.sx = 1; j.sy = 1;
            }
            j.pitch = f.width;
            j.nbands = (j.height + PR_ROWS - 1) / PR_ROWS;
            j.lastpitch = (uint32_t)pl_align_up(j.rowbytes, PLL_ALIGN);
            j.raw = o.raw + (size_t)pass_off[p];
            j.last = data; data += (size_t)j.lastpitch * j.nbands;
            j.prog = r.nprog; r.nprog += j.nbands;
            if (j.nbands > r.max_bands) r.max_bands = j.nbands;
            r.job.push_back(j);
        }
    }
    const size_t st_bytes = pl_align_up(sizeof(int32_t) * n, PLL_ALIGN);
    r.status = pl_align_up(job_bytes * r.job.size(), PLL_ALIGN);
    r.zstatus = r.status + st_bytes;
    r.prog = r.zstatus + st_bytes;
    r.zjobs = r.prog + pl_align_up(sizeof(uint32_t) * r.nprog, PLL_ALIGN);
    r.zeroed = r.zjobs - r.status;
    const size_t head = r.zjobs + pl_align_up(stream_bytes * n, PLL_ALIGN);
    for (size_t i = 0; i < n; i++) {
        PlReadFile &o = r.file[i];
        o.raw += head;
        if (in[i].zbytes != PL_READ_NO_STREAM) o.z += head;
        if (!frames) o.out += head;
    }
    for (PlReadJob &j : r.job) { j.raw += head; j.last += head; }
    r.total = head + data;
    return r;
}

#endif

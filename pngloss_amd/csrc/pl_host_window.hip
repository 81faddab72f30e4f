/*
 * pl_host_window.hip -- batches of HOST images (pl_host_ctx.h has the map of the host files): a window and its stages (stage, upload, the batch,
 * download, scanlines, the deflate / indexed stage), its split into chunks over contexts of one device (batch_host), and all the GPUs of a node
 * (pngloss_hip_multi, deal_over_contexts).  How a window is cut and dealt is pl_plan.h's and pl_deal.h's, where it lies pl_layout.h's.
 */
#include "pl_host_ctx.h"

/* ---- the deflate stage, as window_deflate, window_index and size_search (pl_host_search.hip) state it ---------------------------- */

int deflate_rc(hipError_t e)
{
    return e == hipSuccess ? PNGLOSS_SUCCESS : e == hipErrorInvalidValue ? PNGLOSS_INVALID_ARGUMENT : e == hipErrorOutOfMemory ? PNGLOSS_OUT_OF_MEMORY_ERROR : PNGLOSS_HIP_ERROR;
}

pl_deflate_image deflate_image_of(const void *d_filter_types, const void *d_scanlines, uint32_t pitch, uint32_t rowbytes, uint32_t height,
                                  unsigned char *out, size_t out_capacity)
{
    pl_deflate_image d{};
    d.d_filter_types = static_cast<const uint8_t *>(d_filter_types);
    d.d_scanlines = static_cast<const uint8_t *>(d_scanlines);
    d.pitch = pitch;
    d.rowbytes = rowbytes;
    d.height = height;
    d.out = out;
    d.out_capacity = out_capacity;
    return d;
}

void zstream_clear(pngloss_hip_zstream &z) { z.size = 0; z.color_type = 6; z.blocks[0] = z.blocks[1] = z.blocks[2] = 0; }

void zstream_take(pngloss_hip_zstream &z, const pl_deflate_image &d)
{
    z.size = d.out_size;
    z.blocks[0] = d.blocks_stored; z.blocks[1] = d.blocks_fixed; z.blocks[2] = d.blocks_dynamic;
}

int ensure_copy_stream(pngloss_hip_ctx *ctx)
{
    if (!ctx->copy_stream) PL_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    return PNGLOSS_SUCCESS;
}

namespace {

/* ---- a window of host images (pngloss_hip_optimize_batch_host*): the phases of batch_host_one ------------------------------------ */

/* chunks of one host window take turns at the two phases that are bound by the host's memory (staging in, fanning out), so that
 * chunk k+1 stages while chunk k computes instead of every chunk being in the same phase at the same time */
struct HostTurns { std::atomic<int> stage_turn{ 0 }; std::mutex out_mu; };

/* a few host threads, image i on thread i % nthreads: the copies between the caller's memory and the pinned mirror */
template <class Fn> void for_each_image_on_threads(size_t n, Fn fn)
{
    const unsigned nthreads = (unsigned)std::min<size_t>(12, std::max<size_t>(1, n));
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; t++)
        pool.emplace_back([&, t]() { for (size_t i = t; i < n; i += nthreads) fn(i); });
    for (auto &th : pool) th.join();
}

/* one chunk on its way through the phases: what the caller handed in, where it lies in the arena (pl_layout.h), where the engine emits to */
struct HostWindow {
    pngloss_hip_ctx *ctx;
    const pngloss_hip_host_image *images;
    size_t n;
    pngloss_hip_result *results;
    pngloss_hip_scanlines *lines;
    pngloss_hip_zstream *zs;
    PlWindowLayout lay;
    std::vector<EmitTarget> emits;
    bool indexed = false;           /* option "indexed" on a window that returns zlib streams: the deflate stage also tries colour type 3 (window_index) */
    PlIndexLayout ilay;             /* ... in the index workspace, laid out and grown before anything is enqueued */
    uint32_t index_depth = PLI_DEPTH_8;     /* option "index_depth" beside it: at "auto" and "min" the packed rows lie behind the index workspace */
    PlPackLayout play;
    /* this image's pixels (and filter flags) come back to the caller */
    bool comes_back(size_t i) const
    {
        const bool stream_only = zs && zs[i].data && (zs[i].flags & PNGLOSS_HIP_Z_STREAM_ONLY);
        return lay.im[i].px && !stream_only && results[i].status == 0;
    }
    /* image i's out-flags word (the colour type its scanlines are in): ONE blocking copy per image */
    bool out_flags(size_t i, uint32_t &fl) const { return hipMemcpy(&fl, ctx->h_jobs[i].out_flags, sizeof fl, hipMemcpyDeviceToHost) == hipSuccess; }
};

/* the caller's pixels into the pinned mirror */
void window_stage(const HostWindow &w)
{
    for_each_image_on_threads(w.n, [&](size_t i) {
        if (w.lay.im[i].px) std::memcpy(w.ctx->h_pinned.p + w.lay.im[i].img, w.images[i].rgba, w.lay.im[i].px * 4);
    });
}

/* the engine's view of the arena (descs, w.emits), and the mirror's images up into it */
int window_upload(HostWindow &w, std::vector<pngloss_hip_image_desc> &descs)
{
    pngloss_hip_ctx *ctx = w.ctx;
    char *const arena = ctx->d_arena.p;
    int rc = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < w.n; i++) {
        const PlWindowImage &m = w.lay.im[i];
        descs[i] = pngloss_hip_image_desc{ m.px ? arena + m.img : nullptr, (m.px && w.images[i].row_filters) ? arena + m.flt : nullptr, w.images[i].width, w.images[i].height };
        w.emits[i] = EmitTarget{ m.pitch ? arena + m.ids : nullptr, m.pitch ? arena + m.rows : nullptr, m.pitch };
        /* asynchronous DMA from pinned memory, one per image (the areas between images are filled by the kernels) */
        if (m.px && rc == PNGLOSS_SUCCESS &&
            hipMemcpyAsync(arena + m.img, ctx->h_pinned.p + m.img, m.px * 4, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    }
    if (rc == PNGLOSS_SUCCESS && hipStreamSynchronize(ctx->copy_stream) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    return rc;
}

/* pixels + filter flags of every image that comes back: one copy each (PlWindowImage::span) into the pinned mirror, then fanned out on host threads */
int window_download(const HostWindow &w, HostTurns *turns)
{
    pngloss_hip_ctx *ctx = w.ctx;
    bool any_pixels = false;
    for (size_t i = 0; i < w.n; i++) if (w.comes_back(i)) any_pixels = true;
    if (!any_pixels) return PNGLOSS_SUCCESS;
    for (size_t i = 0; i < w.n; i++) {
        const PlWindowImage &m = w.lay.im[i];
        if (w.comes_back(i) && hipMemcpyAsync(ctx->h_pinned.p + m.img, ctx->d_arena.p + m.img, m.span, hipMemcpyDeviceToHost, ctx->copy_stream) != hipSuccess) return PNGLOSS_HIP_ERROR;
    }
    if (hipStreamSynchronize(ctx->copy_stream) != hipSuccess) return PNGLOSS_HIP_ERROR;
    std::unique_lock<std::mutex> out_lock;
    if (turns) out_lock = std::unique_lock<std::mutex>(turns->out_mu);
    for_each_image_on_threads(w.n, [&](size_t i) {
        if (!w.comes_back(i)) return;
        std::memcpy(w.images[i].rgba, ctx->h_pinned.p + w.lay.im[i].img, w.lay.im[i].px * 4);
        if (w.images[i].row_filters) std::memcpy(w.images[i].row_filters, ctx->h_pinned.p + w.lay.im[i].flt, w.images[i].height);
    });
    return PNGLOSS_SUCCESS;
}

/* the emitted scanlines and filter types straight into the caller's memory, with the colour type they are in */
int window_scanlines(const HostWindow &w)
{
    int rc = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < w.n && rc == PNGLOSS_SUCCESS; i++) {
        if (!w.lay.im[i].px || w.results[i].status != 0 || !w.emits[i].pitch || !w.lines) continue;
        pngloss_hip_scanlines &ln = w.lines[i];
        uint32_t fl = 0;
        if (!w.out_flags(i, fl)) rc = PNGLOSS_HIP_ERROR;
        ln.color_type = pl_color_type_of(fl);
        const size_t rowbytes = (size_t)w.images[i].width * pl_emit_bpp_of(fl);
        if (hipMemcpy(ln.filter_types, w.emits[i].d_ids, w.images[i].height, hipMemcpyDeviceToHost) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
        if (hipMemcpy2D(ln.scanlines, ln.pitch, w.emits[i].d_rows, w.emits[i].pitch, rowbytes, w.images[i].height, hipMemcpyDeviceToHost) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    }
    return rc;
}

/* Option "indexed", behind the truecolour streams of the images `who` (zs[i].size = T is in place): count every image's colours; for the eligible
 * ones build the palette and the index rows and deflate those into a buffer of the window's own -- BOTH candidates are written, and the indexed one
 * replaces the truecolour stream in the caller's buffer where I + overhead < T (pl_index_core.h).  An image that is not eligible costs the count
 * kernel and nothing else, and its stream is the one the call above wrote.  Leaves the palette records of the window in ctx->palette.
 * Option "index_depth" at "auto" adds a third candidate for an image of at most 16 colours -- its index rows packed at min_depth by pl_index_pack,
 * deflated in one more call -- and at "min" puts it in the place of the 8-bit one; which stream is kept is pl_index_core.h's pli_keep_depth, and
 * ctx->index_depth says it.  At "8" nothing here launches or writes anything it did not without that option. */
int window_index(const HostWindow &w, const std::vector<size_t> &who)
{
    pngloss_hip_ctx *ctx = w.ctx;
    pngloss_hip_zstream *zs = w.zs;
    hipStream_t stream = ctx->copy_stream;
    ctx->palette.assign(w.n, pngloss_hip_palette{});
    ctx->index_depth.assign(w.n, pngloss_hip_index_depth{});
    if (who.empty()) return PNGLOSS_SUCCESS;
    char *const base = ctx->d_index.p;
    uint32_t *const d_counts = reinterpret_cast<uint32_t *>(base + w.ilay.counts);
    PliRecord *const d_records = reinterpret_cast<PliRecord *>(base + w.ilay.records);
    std::vector<PlIndexJob> jobs(who.size());
    uint64_t max_pixels = 0;
    for (size_t k = 0; k < who.size(); k++) {
        const size_t i = who[k];
        const PlIndexImage &m = w.ilay.im[i];
        ctx->palette[i].truecolor_bytes = zs[i].size;
        jobs[k] = PlIndexJob{ reinterpret_cast<const uint32_t *>(ctx->d_arena.p + w.lay.im[i].img), (uint64_t)w.lay.im[i].px, w.images[i].width, w.images[i].height,
                              reinterpret_cast<uint64_t *>(base + m.table), d_counts + i, d_records + i, reinterpret_cast<uint8_t *>(base + m.ids),
                              reinterpret_cast<uint8_t *>(base + m.rows), m.pitch, 0 };
        max_pixels = std::max<uint64_t>(max_pixels, w.lay.im[i].px);
    }
    std::vector<uint32_t> counts(w.n, 0);
    PL_CHECK(hipMemsetAsync(base + w.ilay.counts, 0, w.ilay.zeroed, stream));
    PL_CHECK(hipMemsetAsync(base + w.ilay.tables, 0xFF, w.ilay.tables_bytes, stream));
    PL_CHECK(hipMemcpyAsync(base + w.ilay.jobs, jobs.data(), sizeof(PlIndexJob) * jobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(pl_launch_index_count(reinterpret_cast<const PlIndexJob *>(base + w.ilay.jobs), jobs.size(), max_pixels, stream));
    PL_CHECK(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * w.n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    std::vector<PlIndexJob> elig;
    std::vector<size_t> elig_who;
    uint32_t max_height = 0;
    for (size_t k = 0; k < who.size(); k++) {
        const size_t i = who[k];
        ctx->palette[i].colors = pli_colors_of(counts[i]);
        if (counts[i] < 1 || counts[i] > PLI_MAX_COLORS) continue;
        elig.push_back(jobs[k]);
        elig_who.push_back(i);
        max_height = std::max(max_height, w.images[i].height);
    }
    if (elig.empty()) return PNGLOSS_SUCCESS;
    std::vector<PliRecord> records(elig.size());
    PL_CHECK(hipMemcpyAsync(base + w.ilay.jobs, elig.data(), sizeof(PlIndexJob) * elig.size(), hipMemcpyHostToDevice, stream));   /* (the count kernel has read its table: synchronised above) */
    PL_CHECK(pl_launch_index_palette(reinterpret_cast<const PlIndexJob *>(base + w.ilay.jobs), elig.size(), stream));
    PL_CHECK(pl_launch_index_rows(reinterpret_cast<const PlIndexJob *>(base + w.ilay.jobs), elig.size(), max_height, stream));
    /* option "index_depth" at "auto" or "min": the index rows of the images with min_depth < 8 once more, packed at that depth -- one launch, whatever
     * the depths (the counter is the number of entries: held against the record below) */
    constexpr size_t none = ~(size_t)0;
    std::vector<PlPackJob> packs;
    std::vector<size_t> pack_of(elig.size(), none);
    uint32_t pack_height = 0;
    for (size_t k = 0; k < elig.size(); k++) {
        const size_t i = elig_who[k];
        if (!pli_wants_packed(w.index_depth, counts[i])) continue;
        const PlPackImage &m = w.play.im[i];
        pack_of[k] = packs.size();
        packs.push_back(PlPackJob{ elig[k].rows, reinterpret_cast<uint8_t *>(base + m.ids), reinterpret_cast<uint8_t *>(base + m.rows), w.images[i].width, w.images[i].height,
                                   elig[k].pitch, m.pitch, pli_min_depth(counts[i]), 0 });
        pack_height = std::max(pack_height, w.images[i].height);
    }
    if (!packs.empty()) {
        PL_CHECK(hipMemcpyAsync(base + w.play.jobs, packs.data(), sizeof(PlPackJob) * packs.size(), hipMemcpyHostToDevice, stream));
        PL_CHECK(pl_launch_index_pack(reinterpret_cast<const PlPackJob *>(base + w.play.jobs), packs.size(), pack_height, stream));
    }
    for (size_t k = 0; k < elig.size(); k++) PL_CHECK(hipMemcpyAsync(&records[k], elig[k].record, sizeof(PliRecord), hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    /* the candidates: the 8-bit rows of every eligible image (under "min": of those with min_depth 8), then the packed rows, a deflate call each */
    std::vector<pl_deflate_image> dz, dzp(packs.size());
    std::vector<size_t> dz_of(elig.size(), none);
    std::vector<std::vector<unsigned char>> out(elig.size()), outp(packs.size());
    for (size_t k = 0; k < elig.size(); k++) {
        const size_t i = elig_who[k];
        if (records[k].entries != counts[i]) {
            std::fprintf(stderr, "pngloss_hip: indexed: image %zu has %u colours in its table, its counter says %u\n", i, records[k].entries, counts[i]);
            return PNGLOSS_HIP_ERROR;
        }
        const size_t bound = pl_deflate_bound((w.images[i].width + 3) / 4, w.images[i].height);      /* (the bound is stated for 4-byte pixels: width index bytes are at most that many) */
        if (pli_wants_indexed8(w.index_depth, counts[i])) {
            out[k].resize(bound);
            dz_of[k] = dz.size();
            dz.push_back(deflate_image_of(elig[k].ids, elig[k].rows, elig[k].pitch, w.images[i].width, w.images[i].height, out[k].data(), out[k].size()));
        }
        if (pack_of[k] != none) {
            const PlPackJob &pj = packs[pack_of[k]];
            outp[pack_of[k]].resize(bound);
            dzp[pack_of[k]] = deflate_image_of(pj.ids, pj.rows, pj.pitch, pli_packed_rowbytes(pj.width, pj.depth), pj.height, outp[pack_of[k]].data(), bound);
        }
    }
    int rc = dz.empty() ? PNGLOSS_SUCCESS : deflate_rc(pl_deflate_images(dz.data(), dz.size(), nullptr));
    if (rc == PNGLOSS_SUCCESS && !dzp.empty()) rc = deflate_rc(pl_deflate_images(dzp.data(), dzp.size(), nullptr));
    if (rc) return rc;
    for (size_t k = 0; k < elig.size(); k++) {
        const size_t i = elig_who[k];
        pngloss_hip_palette &p = ctx->palette[i];
        pngloss_hip_index_depth &r = ctx->index_depth[i];
        const pl_deflate_image *d8 = dz_of[k] != none ? &dz[dz_of[k]] : nullptr, *dp = pack_of[k] != none ? &dzp[pack_of[k]] : nullptr;
        r.min_depth = pli_min_depth(counts[i]);
        r.indexed8_bytes = d8 ? d8->out_size : 0;
        r.packed_bytes = dp ? dp->out_size : 0;
        p.indexed_bytes = pli_indexed_candidate(w.index_depth, counts[i], r.indexed8_bytes, r.packed_bytes);
        const uint32_t depth = pli_keep_depth(w.index_depth, counts[i], r.indexed8_bytes, r.packed_bytes, p.truecolor_bytes, records[k].trns_entries);     /* (at "8": 8 iff pli_keep_indexed) */
        const pl_deflate_image *kept = depth == 8 ? d8 : dp;
        if (!depth || kept->out_size > zs[i].capacity) continue;
        r.bit_depth = depth;
        p.entries = records[k].entries;
        p.trns_entries = records[k].trns_entries;
        for (uint32_t e = 0; e < p.entries; e++) {
            const uint32_t word = records[k].words[e];
            p.rgb[e][0] = (uint8_t)word; p.rgb[e][1] = (uint8_t)(word >> 8); p.rgb[e][2] = (uint8_t)(word >> 16);
            p.alpha[e] = (uint8_t)(word >> 24);
        }
        std::memcpy(zs[i].data, kept->out, kept->out_size);
        zstream_take(zs[i], *kept);
        zs[i].color_type = 3;
    }
    return PNGLOSS_SUCCESS;
}

/* the emitted scanlines through the device deflate into the caller's zlib streams */
int window_deflate(const HostWindow &w)
{
    pngloss_hip_ctx *ctx = w.ctx;
    pngloss_hip_zstream *zs = w.zs;
    int rc = PNGLOSS_SUCCESS;
    /* the colour type decides the scanline length, so it is fetched before the deflate stage is laid out */
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<pl_deflate_image> dz;
    std::vector<size_t> who;
    for (size_t i = 0; i < w.n && rc == PNGLOSS_SUCCESS; i++) {
        zstream_clear(zs[i]);
        if (!w.emits[i].pitch || w.results[i].status != 0) continue;
        uint32_t fl = 0;
        if (!w.out_flags(i, fl)) { rc = PNGLOSS_HIP_ERROR; break; }
        zs[i].color_type = pl_color_type_of(fl);
        dz.push_back(deflate_image_of(w.emits[i].d_ids, w.emits[i].d_rows, w.emits[i].pitch, w.images[i].width * pl_emit_bpp_of(fl), w.images[i].height, zs[i].data, zs[i].capacity));
        who.push_back(i);
    }
    if (rc == PNGLOSS_SUCCESS && !dz.empty()) {
        rc = deflate_rc(pl_deflate_images(dz.data(), dz.size(), nullptr));
        for (size_t k = 0; k < dz.size() && rc == PNGLOSS_SUCCESS; k++) zstream_take(zs[who[k]], dz[k]);
    }
    if (rc == PNGLOSS_SUCCESS && w.indexed) rc = window_index(w, who);
    ctx->deflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ctx->hooks.debug_seam) std::fprintf(stderr, "pngloss_hip: host window: deflate stage %.1f ms for %zu images\n", ctx->deflate_ms, dz.size());
    return rc;
}

int batch_host_one(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, unsigned quantization_strength,
                   long bleed_divider, Measure measure, pngloss_hip_result *results, pngloss_hip_scanlines *lines,
                   pngloss_hip_zstream *zs, HostTurns *turns = nullptr, int my_turn = 0)
{
    /* whatever happens below, the next chunk must get its turn */
    struct TurnGuard { HostTurns *t; int mine; bool passed = false; void pass() { if (t && !passed) { while (t->stage_turn.load(std::memory_order_acquire) != mine) std::this_thread::yield(); t->stage_turn.store(mine + 1, std::memory_order_release); passed = true; } } ~TurnGuard() { pass(); } } turn{ turns, my_turn };
    if (!ctx || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<PlWindowIn> in(n);
    for (size_t i = 0; i < n; i++) {
        if (images[i].width && images[i].height && !images[i].rgba) return PNGLOSS_INVALID_ARGUMENT;
        in[i] = PlWindowIn{ images[i].width, images[i].height, images[i].row_filters != nullptr,
                            (lines && lines[i].scanlines && lines[i].filter_types) || (zs && zs[i].data) };
    }
    HostWindow w{ ctx, images, n, results, lines, zs, pl_window_layout(in), std::vector<EmitTarget>(n) };
    for (size_t i = 0; i < n; i++)
        if (w.lay.im[i].pitch && lines && lines[i].pitch < (size_t)images[i].width * 4) return PNGLOSS_INVALID_ARGUMENT;
    /* persistent arena + pinned staging of the same layout; images are staged by a few host threads and go up as asynchronous
     * copies from pinned memory, one per image (pageable per-image copies were 0.33 s of a 1.6 s window of 256 720p files in round 1).
     * Copies and kernels of a context run on its own non-blocking stream, so that two contexts (the two halves of a window,
     * batch_host) overlap: one half's transfers with the other half's kernels. */
    const auto ta0 = std::chrono::steady_clock::now();
    int rc = ctx->d_arena.grow(w.lay.total, 8);
    if (rc == PNGLOSS_SUCCESS) rc = ctx->h_pinned.grow(w.lay.mirrored, 8);
    if (rc == PNGLOSS_SUCCESS && zs && measure.indexed) {
        std::vector<uint32_t> width, height;
        batch_dims(images, n, width, height);
        w.indexed = true;
        w.ilay = pl_index_layout(width, height, sizeof(PlIndexJob), sizeof(PliRecord));
        w.index_depth = measure.index_depth;
        if (w.index_depth != PLI_DEPTH_8) w.play = pl_index_pack_layout(width, height, w.ilay.total, sizeof(PlPackJob));
        rc = ctx->d_index.grow(w.index_depth != PLI_DEPTH_8 ? w.play.total : w.ilay.total, 8);
    }
    if (rc == PNGLOSS_SUCCESS) rc = ensure_copy_stream(ctx);
    if (rc) return rc;
    if (ctx->hooks.debug_seam) std::fprintf(stderr, "pngloss_hip: host window chunk %d: arena %zu MB + pinned mirror %zu MB ready after %.1f ms\n", my_turn, w.lay.total >> 20, w.lay.mirrored >> 20, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta0).count());
    std::vector<pngloss_hip_image_desc> descs(n);
    if (turns) while (turns->stage_turn.load(std::memory_order_acquire) != my_turn) std::this_thread::yield();
    const auto tu0 = std::chrono::steady_clock::now();
    window_stage(w);
    turn.pass();                                              /* the next chunk may stage while this one uploads and computes */
    rc = window_upload(w, descs);
    ctx->upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count();
    std::vector<pngloss_hip_result> own_results;
    if (!results) { own_results.resize(n ? n : 1); results = w.results = own_results.data(); }
    if (rc == PNGLOSS_SUCCESS) {
        BatchCall call{ quantization_strength, bleed_divider, ctx->copy_stream, measure };
        call.sync_call = true;                  /* (finish follows at once: no device-side wait on the copy stream, run_seg_engine) */
        call.emits = w.emits.data();
        rc = enqueue(ctx, descs.data(), n, call);
    }
    if (rc == PNGLOSS_SUCCESS) rc = finish(ctx, results, n);
    /* a row without an acceptable filter (device status 65, pngloss_image.c:268-271) fails THAT image only: the others of
     * the batch are downloaded and the call reports PNGLOSS_INTERNAL_ABORT with the per-image status in results[] */
    const bool some_aborted = rc == PNGLOSS_INTERNAL_ABORT;
    if (some_aborted) rc = PNGLOSS_SUCCESS;
    const auto td0 = std::chrono::steady_clock::now();
    if (rc == PNGLOSS_SUCCESS) rc = window_download(w, turns);
    if (rc == PNGLOSS_SUCCESS) rc = window_scanlines(w);
    ctx->download_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0).count();
    if (ctx->hooks.debug_seam)
        std::fprintf(stderr, "pngloss_hip: host window chunk %d: %zu images, wait+stage+upload %.1f ms, engine %.1f ms (enqueue..finish %.1f ms), download+fan-out %.1f ms\n", my_turn, n, ctx->upload_ms, ctx->engine_ms,
                     std::chrono::duration<double, std::milli>(td0 - tu0).count() - ctx->upload_ms, ctx->download_ms);
    if (zs && rc == PNGLOSS_SUCCESS) rc = window_deflate(w);
    if (rc == PNGLOSS_HIP_ERROR) std::fprintf(stderr, "pngloss_hip: batch transfer or kernel failure: %s\n", hipGetErrorString(hipGetLastError()));
    if (rc == PNGLOSS_SUCCESS && some_aborted) rc = PNGLOSS_INTERNAL_ABORT;
    return rc;
}

} // namespace

/* A window of host images: in two halves on two contexts of the same device, a host thread each, when it is large enough -- the
 * second half is staged and uploaded while the first one computes, the first one is downloaded while the second one computes
 * (profiles/r02_host_seam.txt: staging + PCIe were 0.26 s next to a 0.28 s engine for 256 x 720p, one after the other).  The deflate
 * stage (zs) keeps its single pass: it sorts the whole window's scanlines as one stream. */
int batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, unsigned quantization_strength,
               long bleed_divider, Measure measure, pngloss_hip_result *results, pngloss_hip_scanlines *lines,
               pngloss_hip_zstream *zs)
{
    if (!ctx || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    ctx->split_last = false;
    /* chunks, each on its own context and stream, staggered by the staging turns (pl_host_window_chunks) */
    size_t K = pl_host_window_chunks(n, ctx->hooks, zs != nullptr);
    if (K <= 1) return batch_host_one(ctx, images, n, quantization_strength, bleed_divider, measure, results, lines, zs);
    while (ctx->peers.size() < K - 1) {
        pngloss_hip_ctx *p = pngloss_hip_create(ctx->device);
        if (!p) break;
        ctx->peers.push_back(p);
    }
    K = std::min(K, ctx->peers.size() + 1);
    if (K <= 1) return batch_host_one(ctx, images, n, quantization_strength, bleed_divider, measure, results, lines, zs);
    std::vector<uint64_t> pixels(n);
    for (size_t i = 0; i < n; i++) pixels[i] = (uint64_t)images[i].width * images[i].height;
    const std::vector<size_t> first = pl_host_window_cut(pixels, K);
    std::vector<pngloss_hip_result> own;
    if (!results) { own.resize(n); results = own.data(); }
    HostTurns turns;
    std::vector<int> rcs(K, PNGLOSS_SUCCESS);
    auto run_chunk = [&](size_t c) {
        pngloss_hip_ctx *cc = c == 0 ? ctx : ctx->peers[c - 1];
        rcs[c] = batch_host_one(cc, images + first[c], first[c + 1] - first[c], quantization_strength, bleed_divider, measure, results + first[c],       /* (every chunk measures the same) */
                                lines ? lines + first[c] : nullptr, nullptr, &turns, (int)c);
    };
    std::vector<std::thread> others;
    for (size_t c = 1; c < K; c++) others.emplace_back(run_chunk, c);
    run_chunk(0);
    for (auto &t : others) t.join();
    ctx->split_last = true;
    ctx->chunk_first.assign(first.begin(), first.begin() + (long)K);
    for (size_t c = 1; c < K; c++) {
        pngloss_hip_ctx *p = ctx->peers[c - 1];
        ctx->engine_ms = std::max(ctx->engine_ms, p->engine_ms);
        ctx->total_ms = std::max(ctx->total_ms, p->total_ms);
        ctx->upload_ms += p->upload_ms; ctx->download_ms += p->download_ms;
    }
    return pl_fold_rc(rcs);
}

/* A batch of host images over the contexts of the node, the one shape of every pngloss_hip_multi_optimize_batch_host* call: the split, a host thread per
 * context that got an image, share(context, its images as a HostSubset) -> code on each, results / scanlines / streams back in input order, the codes folded
 * (pl_deal.h).  indexes_last: the call leaves a last batch per context that pngloss_hip_multi_last_* index through `where`; else `where` is cleared (the
 * searches' records are in their reports). */
int deal_over_contexts(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, pngloss_hip_result *results,
                       pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams, bool indexes_last,
                       const std::function<int(pngloss_hip_ctx *, HostSubset &)> &share)
{
    const int parts = (int)m->ctx.size();
    std::vector<int> owner(n ? n : 1, 0);
    pngloss_hip_multi_split(images, n, parts, owner.data());
    PlDeal deal = pl_deal(owner.data(), n, parts);
    if (indexes_last) m->where.swap(deal.where);
    else m->where.clear();
    std::vector<int> rcs((size_t)parts, PNGLOSS_SUCCESS);
    std::vector<std::thread> pool;
    for (size_t p2 = 0; p2 < (size_t)parts; p2++) {
        if (deal.part[p2].empty()) continue;
        pool.emplace_back([&, p2]() {
            HostSubset mine(deal.part[p2], images, scanlines, streams);
            rcs[p2] = share(m->ctx[p2], mine);
            mine.scatter(results, scanlines, streams);
        });
    }
    for (auto &th : pool) th.join();
    return pl_fold_rc(rcs);
}

/* ================================================================================================ C ABI */

extern "C" {

int pngloss_hip_optimize_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                    unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results)
{
    return batch_host(ctx, images, n, quantization_strength, bleed_divider, measure_of_options(ctx), results, nullptr);
}

int pngloss_hip_optimize_batch_host_emit(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                         unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                         pngloss_hip_scanlines *scanlines)
{
    return batch_host(ctx, images, n, quantization_strength, bleed_divider, measure_of_options(ctx), results, scanlines);
}

int pngloss_hip_optimize_batch_host_zlib(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                         unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                         pngloss_hip_zstream *streams)
{
    if (!streams && n) return PNGLOSS_INVALID_ARGUMENT;
    return batch_host(ctx, images, n, quantization_strength, bleed_divider, measure_of_options(ctx), results, nullptr, streams);
}

size_t pngloss_hip_zlib_bound(uint32_t width, uint32_t height) { return pl_deflate_bound(width, height); }

/* ---- all the GPUs of the node (replaces the one-file-at-a-time loop of the reference's src/pngloss.c:173-208 for a whole
 * node): one context per device, images dealt out by size (longest-processing-time first), one host thread per context,
 * results back in input order.  No collective: images are independent. ---------------------------------------------- */
void pngloss_hip_multi_split(const pngloss_hip_host_image *images, size_t n, int parts, int *owner)
{
    std::vector<uint64_t> pixels(n);
    for (size_t i = 0; i < n; i++) pixels[i] = (uint64_t)images[i].width * images[i].height;
    const std::vector<int> own = pl_deal_owners(pixels, parts);      /* (the LPT rule: pl_deal.h) */
    std::copy(own.begin(), own.end(), owner);
}

pngloss_hip_multi *pngloss_hip_multi_create(const char *devices)
{
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) {
        std::fprintf(stderr, "pngloss_hip: no HIP device available\n");
        return nullptr;
    }
    if (!devices || !*devices) devices = std::getenv("PNGLOSS_DEVICES");
    std::vector<int> want;
    if (devices && *devices) {
        const char *p2 = devices;
        while (*p2) {
            char *end = nullptr;
            const long d = std::strtol(p2, &end, 10);
            if (end == p2 || d < 0 || d >= visible) {
                std::fprintf(stderr, "pngloss_hip: bad device list \"%s\" (%d device(s) visible)\n", devices, visible);
                return nullptr;
            }
            want.push_back((int)d);
            p2 = end;
            while (*p2 == ',' || *p2 == ' ') p2++;
        }
    } else {
        for (int d = 0; d < visible; d++) want.push_back(d);
    }
    if (want.empty()) return nullptr;
    pngloss_hip_multi *m = new (std::nothrow) pngloss_hip_multi;
    if (!m) return nullptr;
    for (int d : want) {
        pngloss_hip_ctx *c = pngloss_hip_create(d);
        if (!c) { pngloss_hip_multi_destroy(m); return nullptr; }
        m->ctx.push_back(c);
    }
    return m;
}

void pngloss_hip_multi_destroy(pngloss_hip_multi *m)
{
    if (!m) return;
    for (pngloss_hip_ctx *c : m->ctx) pngloss_hip_destroy(c);
    delete m;
}

int pngloss_hip_multi_count(const pngloss_hip_multi *m) { return m ? (int)m->ctx.size() : 0; }

int pngloss_hip_multi_optimize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                          unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                          pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams)
{
    if (!m || m->ctx.empty() || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    return deal_over_contexts(m, images, n, results, scanlines, streams, true, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        return batch_host(ctx, mine.images.data(), mine.n(), quantization_strength, bleed_divider, measure_of_options(ctx), mine.results.data(), mine.lines(), mine.zs());
    });
}

} /* extern "C" */

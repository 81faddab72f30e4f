/*
 * pl_host_quant.hip -- the host side of the colour quantiser (include/pngloss_hip_quant.h, pngloss_hip_dither.h; pl_host_ctx.h has the map of the
 * host files): the argument checks, the workspace (pl_layout.h: pl_quant_layout, pl_dither_layout), the median cut between the two synchronisations
 * (pl_quant_core.h), the launches of pl_quant.hip, of pl_dither.hip in place of the remap pass when the call dithers, and of the kernels it borrows -- pl_index_count / pl_index_palette for the colours before and after, pl_distort for the record --, and the host
 * form over the contexts of a node (deal_over_contexts).  The space of a call (include/pngloss_hip_quant_space.h; its entry points are in
 * pl_host_quant_space.hip) travels in the workspace record: every stage asks b.ws.visible which twin of a kernel it launches.
 */
#include "pl_host_ctx.h"

int check_quant_params(const pngloss_hip_quant_params2 *params)
{
    if (!params || params->max_colors < PLQ_MIN_COLORS || params->max_colors > PLQ_MAX_COLORS || params->rounds > PLQ_MAX_ROUNDS) return PNGLOSS_INVALID_ARGUMENT;
    if (params->dither > PNGLOSS_HIP_DITHER_FLOYD_STEINBERG || params->reserved) return PNGLOSS_INVALID_ARGUMENT;
    return PNGLOSS_SUCCESS;
}

int check_quant_pixels(const uint32_t *width, const uint32_t *height, size_t n, const void *const *pixels_of)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t px = (uint64_t)width[i] * height[i];
        if (px && !pixels_of[i]) return PNGLOSS_INVALID_ARGUMENT;
        if (!plq_pixels_ok(px)) return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_SUCCESS;
}

namespace {

/* the old record as the new one: no dithering */
const pngloss_hip_quant_params2 *widen(const pngloss_hip_quant_params *params, pngloss_hip_quant_params2 &wide)
{
    if (!params) return nullptr;
    wide = pngloss_hip_quant_params2{ params->max_colors, params->rounds, PNGLOSS_HIP_DITHER_NONE, 0 };
    return &wide;
}

template <class Image> int check_quant_sizes(const Image *images, size_t n, const void *const *pixels_of)
{
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    return check_quant_pixels(width.data(), height.data(), n, pixels_of);
}

PlQuantLayout quant_layout_of(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs)
{
    return pl_quant_layout(width, height, inputs, sizeof(PlIndexJob), sizeof(PlQuantJob), sizeof(PlDistortJob), sizeof(PliRecord), sizeof(PlDistortRecord));
}

} // namespace

QuantWorkspace quant_workspace_of(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs, const pngloss_hip_quant_params2 &params,
                                  uint32_t space)
{
    QuantWorkspace ws;
    ws.lay = quant_layout_of(width, height, inputs);
    ws.visible = space == PNGLOSS_HIP_QUANT_SPACE_VISIBLE;
    ws.dithers = params.dither == PNGLOSS_HIP_DITHER_FLOYD_STEINBERG;
    if (ws.dithers) ws.dither = pl_dither_layout(width, ws.lay.total, sizeof(PlDitherJob));
    return ws;
}

/* ---- the stages of a call (QuantBatch, pl_host_ctx.h): quantize_on below runs them once each, the colour-count search of
 * pl_host_quant_target.hip the first once, the second once per round and the third once ---- */

/* The colours and the histogram of every image, and the one synchronisation the median cut needs.  reports[i]: cleared, exact for an image without
 * pixels, colors_in of the others. */
int quant_survey(QuantBatch &b, pngloss_hip_quant_report *reports)
{
    const PlQuantLayout &lay = b.ws.lay;
    const size_t n = b.img.size();
    char *const base = b.base();
    uint32_t *const d_counts = reinterpret_cast<uint32_t *>(base + lay.counts);
    PliRecord *const d_records = reinterpret_cast<PliRecord *>(base + lay.records);
    for (size_t i = 0; i < n; i++) {
        reports[i] = pngloss_hip_quant_report{};
        reports[i].exact = 1;                       /* (an image without pixels: exact, no entries) */
        const uint64_t px = (uint64_t)b.width[i] * b.height[i];
        if (!px) continue;
        const PlQuantImage &m = lay.im[i];
        b.live.push_back(i);
        b.ijobs.push_back(PlIndexJob{ b.img[i], px, b.width[i], b.height[i], reinterpret_cast<uint64_t *>(base + m.table), d_counts + i, d_records + i, nullptr, nullptr, 0, 0 });
        b.qjobs.push_back(PlQuantJob{ b.img[i], reinterpret_cast<uint32_t *>(base + m.out), px, reinterpret_cast<uint32_t *>(base + m.hist),
                                      reinterpret_cast<uint32_t *>(base + m.pal), reinterpret_cast<uint64_t *>(base + m.acc), 0, 0 });
        b.max_pixels = std::max(b.max_pixels, px);
    }
    b.counts.assign(n, 0);
    if (b.live.empty()) return PNGLOSS_SUCCESS;
    hipStream_t stream = b.stream;
    b.hists.resize(b.live.size() * (size_t)PLQ_BINS);
    PL_CHECK(hipMemsetAsync(base + lay.counts, 0, lay.zeroed, stream));
    PL_CHECK(hipMemsetAsync(base + lay.tables, 0xFF, lay.tables_bytes, stream));
    PL_CHECK(hipMemsetAsync(base + lay.hists, 0, lay.hists_bytes, stream));
    PL_CHECK(hipMemcpyAsync(base + lay.index_jobs, b.ijobs.data(), sizeof(PlIndexJob) * b.ijobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(hipMemcpyAsync(base + lay.quant_jobs, b.qjobs.data(), sizeof(PlQuantJob) * b.qjobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(pl_launch_index_count(b.d_ijobs(), b.ijobs.size(), b.max_pixels, stream));
    PL_CHECK(pl_launch_quant_hist(b.d_qjobs(), b.qjobs.size(), b.max_pixels, stream, b.ws.visible));
    PL_CHECK(hipMemcpyAsync(b.counts.data(), d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
    for (size_t k = 0; k < b.live.size(); k++)
        PL_CHECK(hipMemcpyAsync(b.hists.data() + k * (size_t)PLQ_BINS, b.qjobs[k].hist, PLL_QUANT_HIST, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    for (size_t i : b.live) reports[i].colors_in = pli_colors_of(b.counts[i]);
    return PNGLOSS_SUCCESS;
}

/* The initial palette of image live[k] at `colors` entries at most, into its place in `pals` (PLQ_MAX_COLORS words per image of the batch) and its
 * length into the image's job */
int quant_first_palette(QuantBatch &b, size_t k, uint32_t colors, std::vector<uint32_t> &pals)
{
    const size_t i = b.live[k];
    const std::vector<uint32_t> first = plq_median_cut(b.hists.data() + k * (size_t)PLQ_BINS, colors);
    if (first.empty() || first.size() > colors) {
        std::fprintf(stderr, "pngloss_hip: quantize: image %zu: a histogram without pixels\n", i);
        return PNGLOSS_HIP_ERROR;
    }
    std::fill(pals.begin() + (long)(i * (size_t)PLQ_MAX_COLORS), pals.begin() + (long)((i + 1) * (size_t)PLQ_MAX_COLORS), 0u);
    std::copy(first.begin(), first.end(), pals.begin() + (long)(i * (size_t)PLQ_MAX_COLORS));
    b.qjobs[k].entries = (uint32_t)first.size();
    return PNGLOSS_SUCCESS;
}

/* The palettes up, the job table of the images live[k], k in `work`, in place (`jobs` gets it: the later launches are sized by it), and `rounds`
 * refinement rounds over them.  (The histogram kernel has read its table: quant_survey synchronised.) */
int quant_refine(QuantBatch &b, const std::vector<size_t> &work, const std::vector<uint32_t> &pals, uint32_t rounds, std::vector<PlQuantJob> &jobs, uint64_t &work_pixels)
{
    jobs.clear();
    work_pixels = 0;
    for (size_t k : work) {
        jobs.push_back(b.qjobs[k]);
        work_pixels = std::max(work_pixels, b.qjobs[k].pixels);
    }
    if (jobs.empty()) return PNGLOSS_SUCCESS;
    char *const base = b.base();
    PL_CHECK(hipMemcpyAsync(base + b.ws.lay.pals, pals.data(), PLL_QUANT_PAL * b.img.size(), hipMemcpyHostToDevice, b.stream));
    PL_CHECK(hipMemcpyAsync(base + b.ws.lay.quant_jobs, jobs.data(), sizeof(PlQuantJob) * jobs.size(), hipMemcpyHostToDevice, b.stream));
    for (uint32_t round = 0; round < rounds; round++) {
        PL_CHECK(pl_launch_quant_assign(b.d_qjobs(), jobs.size(), work_pixels, b.stream, b.ws.visible));
        PL_CHECK(pl_launch_quant_update(b.d_qjobs(), jobs.size(), b.stream));
    }
    return PNGLOSS_SUCCESS;
}

/* The dither pass over the images live[k], k in `work`, into their `out`, with the palettes that lie on the device */
int quant_dither(QuantBatch &b, const std::vector<size_t> &work)
{
    std::vector<PlDitherJob> dither;
    char *const base = b.base();
    for (size_t k : work) {
        const size_t i = b.live[k];
        dither.push_back(PlDitherJob{ b.img[i], b.qjobs[k].out, b.qjobs[k].pal, reinterpret_cast<PlfErr *>(base + b.ws.dither.line[i]), b.width[i], b.height[i], b.qjobs[k].entries, 0 });
    }
    if (dither.empty()) return PNGLOSS_SUCCESS;
    PL_CHECK(hipMemcpyAsync(base + b.ws.dither.jobs, dither.data(), sizeof(PlDitherJob) * dither.size(), hipMemcpyHostToDevice, b.stream));
    PL_CHECK(pl_launch_dither(reinterpret_cast<const PlDitherJob *>(base + b.ws.dither.jobs), dither.size(), b.stream, b.ws.visible));
    return PNGLOSS_SUCCESS;
}

/* The tail of a call.  `jobs`: the table quant_refine left in place, whose images get the remap pass (or the dither pass: `pass`, the same images
 * as indices into live) into their `out`.  Then for every image the record of (input, output) while both exist -- the output of an image whose
 * reports[i].exact is 0 is its `out` --, the output over the input, and the palette that is reported; allowed[i]: the colours image i may have. */
int quant_close(QuantBatch &b, const std::vector<PlQuantJob> &jobs, uint64_t work_pixels, const std::vector<size_t> &pass, const std::vector<uint32_t> &allowed,
                pngloss_hip_quant_report *reports)
{
    const PlQuantLayout &lay = b.ws.lay;
    const size_t n = b.img.size();
    char *const base = b.base();
    hipStream_t stream = b.stream;
    uint32_t *const d_counts = reinterpret_cast<uint32_t *>(base + lay.counts);
    PliRecord *const d_records = reinterpret_cast<PliRecord *>(base + lay.records);
    PlDistortRecord *const d_distort = reinterpret_cast<PlDistortRecord *>(base + lay.distort_records);
    const PlDistortJob *const d_djobs = reinterpret_cast<const PlDistortJob *>(base + lay.distort_jobs);
    if (b.live.empty()) return PNGLOSS_SUCCESS;
    std::vector<PlDistortJob> djobs(b.live.size());
    for (size_t k = 0; k < b.live.size(); k++) {
        const size_t i = b.live[k];
        djobs[k] = PlDistortJob{ b.img[i], reports[i].exact ? b.img[i] : b.qjobs[k].out, b.qjobs[k].pixels, d_distort + i };
    }
    if (!jobs.empty()) {
        if (b.ws.dithers) {
            const int rc = quant_dither(b, pass);
            if (rc) return rc;
        } else {
            PL_CHECK(pl_launch_quant_remap(b.d_qjobs(), jobs.size(), work_pixels, stream, b.ws.visible));
        }
    }
    /* the record of (input, output) while both exist -- in the premultiplied space the visible-mode one, which counts `pixels` itself into records
     * that are zero (quant_survey zeroed them, or the search did before its close) --, then the output over the input */
    PL_CHECK(hipMemcpyAsync(base + lay.distort_jobs, djobs.data(), sizeof(PlDistortJob) * djobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(pl_launch_distort(d_djobs, djobs.size(), b.max_pixels, stream, b.ws.visible));
    for (size_t k = 0; k < b.live.size(); k++)
        if (!reports[b.live[k]].exact)
            PL_CHECK(hipMemcpyAsync(const_cast<uint32_t *>(b.qjobs[k].img), b.qjobs[k].out, (size_t)b.qjobs[k].pixels * 4, hipMemcpyDeviceToDevice, stream));
    /* the palette that is reported: the colours of the image as it is now, counted and ordered by the indexed side's own kernels */
    PL_CHECK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * n, stream));
    PL_CHECK(hipMemsetAsync(base + lay.tables, 0xFF, lay.tables_bytes, stream));
    PL_CHECK(pl_launch_index_count(b.d_ijobs(), b.ijobs.size(), b.max_pixels, stream));
    PL_CHECK(pl_launch_index_palette(b.d_ijobs(), b.ijobs.size(), stream));
    std::vector<PliRecord> records(n);
    std::vector<PlDistortRecord> distort(n);
    PL_CHECK(hipMemcpyAsync(b.counts.data(), d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(records.data(), d_records, sizeof(PliRecord) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(distort.data(), d_distort, sizeof(PlDistortRecord) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    for (size_t i : b.live) {
        pngloss_hip_quant_report &rep = reports[i];
        if (records[i].entries != b.counts[i] || b.counts[i] < 1 || b.counts[i] > allowed[i]) {
            std::fprintf(stderr, "pngloss_hip: quantize: image %zu has %u colours in its table, its counter says %u, %u were allowed\n", i, records[i].entries, b.counts[i], allowed[i]);
            return PNGLOSS_HIP_ERROR;
        }
        rep.entries = records[i].entries;
        std::copy(records[i].words, records[i].words + rep.entries, rep.palette);
        std::memcpy(&rep.distortion, &distort[i], sizeof rep.distortion);
    }
    return PNGLOSS_SUCCESS;
}

namespace {

/* The images img[0 .. n) (device, width[i] * height[i] words each) quantised in place, in the workspace ctx->d_quant, which the caller has grown to
 * ws.total().  Waits for `stream` twice: behind the colour counts and the histograms, and at the end. */
int quantize_on(pngloss_hip_ctx *ctx, const QuantWorkspace &ws, const std::vector<uint32_t *> &img, const std::vector<uint32_t> &width,
                const std::vector<uint32_t> &height, const pngloss_hip_quant_params2 &params, pngloss_hip_quant_report *reports, hipStream_t stream)
{
    QuantBatch b{ ctx, ws, img, width, height, stream };
    int rc = quant_survey(b, reports);
    if (rc || b.live.empty()) return rc;
    /* exact images leave here; the others get their initial palette */
    std::vector<size_t> work;
    std::vector<uint32_t> pals(img.size() * (size_t)PLQ_MAX_COLORS, 0);
    for (size_t k = 0; k < b.live.size(); k++) {
        const size_t i = b.live[k];
        reports[i].exact = reports[i].colors_in <= params.max_colors;
        if (reports[i].exact) continue;
        rc = quant_first_palette(b, k, params.max_colors, pals);
        if (rc) return rc;
        work.push_back(k);
    }
    std::vector<PlQuantJob> jobs;
    uint64_t work_pixels = 0;
    rc = quant_refine(b, work, pals, params.rounds, jobs, work_pixels);
    if (rc) return rc;
    return quant_close(b, jobs, work_pixels, work, std::vector<uint32_t>(img.size(), params.max_colors), reports);
}

/* the share of one context in the host form: its images up into the workspace, quantised there, the changed ones back */
int quantize_host_share(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 &params, uint32_t space,
                        pngloss_hip_quant_report *reports)
{
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    const QuantWorkspace ws = quant_workspace_of(width, height, true, params, space);
    const PlQuantLayout &lay = ws.lay;
    int rc = ctx->d_quant.grow(ws.total(), 8);
    if (rc == PNGLOSS_SUCCESS) rc = ensure_copy_stream(ctx);
    if (rc) return rc;
    hipStream_t stream = ctx->copy_stream;
    std::vector<uint32_t *> img(n);
    for (size_t i = 0; i < n; i++) {
        const size_t bytes = (size_t)width[i] * height[i] * 4;
        img[i] = reinterpret_cast<uint32_t *>(ctx->d_quant.p + lay.im[i].in);
        if (bytes) PL_CHECK(hipMemcpyAsync(img[i], images[i].rgba, bytes, hipMemcpyHostToDevice, stream));
    }
    rc = quantize_on(ctx, ws, img, width, height, params, reports, stream);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
        const size_t bytes = (size_t)width[i] * height[i] * 4;
        if (bytes && !reports[i].exact) PL_CHECK(hipMemcpyAsync(images[i].rgba, img[i], bytes, hipMemcpyDeviceToHost, stream));
    }
    PL_CHECK(hipStreamSynchronize(stream));
    return PNGLOSS_SUCCESS;
}

} // namespace

/* every form of pngloss_hip_quantize_batch; space: PNGLOSS_HIP_QUANT_SPACE_*, checked by the caller */
int quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                   pngloss_hip_quant_report *reports, void *stream_)
{
    if (!ctx || (n && (!images || !reports)) || check_quant_params(params)) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<const void *> pixels_of(n);
    for (size_t i = 0; i < n; i++) pixels_of[i] = images[i].d_rgba;
    if (check_quant_sizes(images, n, pixels_of.data())) return PNGLOSS_INVALID_ARGUMENT;
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    const QuantWorkspace ws = quant_workspace_of(width, height, false, *params, space);
    const int rc = ctx->d_quant.grow(ws.total(), 8);
    if (rc) return rc;
    std::vector<uint32_t *> img(n);
    for (size_t i = 0; i < n; i++) img[i] = static_cast<uint32_t *>(images[i].d_rgba);
    return quantize_on(ctx, ws, img, width, height, *params, reports, static_cast<hipStream_t>(stream_));
}

/* every form of pngloss_hip_multi_quantize_batch_host */
int multi_quantize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                              pngloss_hip_quant_report *reports)
{
    if (!m || m->ctx.empty() || (n && (!images || !reports)) || check_quant_params(params)) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<const void *> pixels_of(n);
    for (size_t i = 0; i < n; i++) pixels_of[i] = images[i].rgba;
    if (check_quant_sizes(images, n, pixels_of.data())) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    /* (no last batch to index: the records are in the reports) */
    return deal_over_contexts(m, images, n, nullptr, nullptr, nullptr, false, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        std::vector<pngloss_hip_quant_report> own(mine.n());
        const int rc = quantize_host_share(ctx, mine.images.data(), mine.n(), *params, space, own.data());
        for (size_t k = 0; k < mine.n(); k++) reports[mine.who[k]] = own[k];
        return rc;
    });
}

extern "C" {

int pngloss_hip_quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params *params,
                               pngloss_hip_quant_report *reports, void *stream)
{
    pngloss_hip_quant_params2 wide;
    return quantize_batch(ctx, images, n, widen(params, wide), PNGLOSS_HIP_QUANT_SPACE_RGBA, reports, stream);
}

int pngloss_hip_multi_quantize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params *params,
                                          pngloss_hip_quant_report *reports)
{
    pngloss_hip_quant_params2 wide;
    return multi_quantize_batch_host(m, images, n, widen(params, wide), PNGLOSS_HIP_QUANT_SPACE_RGBA, reports);
}

int pngloss_hip_quantize_batch2(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
                                pngloss_hip_quant_report *reports, void *stream)
{
    return quantize_batch(ctx, images, n, params, PNGLOSS_HIP_QUANT_SPACE_RGBA, reports, stream);
}

int pngloss_hip_multi_quantize_batch_host2(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params,
                                           pngloss_hip_quant_report *reports)
{
    return multi_quantize_batch_host(m, images, n, params, PNGLOSS_HIP_QUANT_SPACE_RGBA, reports);
}

} /* extern "C" */

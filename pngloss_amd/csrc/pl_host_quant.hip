/*
 * pl_host_quant.hip -- the host side of the colour quantiser (include/pngloss_hip_quant.h, pngloss_hip_dither.h; pl_host_ctx.h has the map of the
 * host files): the argument checks, the workspace (pl_layout.h: pl_quant_layout, pl_dither_layout), the median cut between the two synchronisations
 * (pl_quant_core.h), the launches of pl_quant.hip, of pl_dither.hip in place of the remap pass when the call dithers, and of the kernels it borrows -- pl_index_count / pl_index_palette for the colours before and after, pl_distort for the record --, and the host
 * form over the contexts of a node (deal_over_contexts).
 */
#include "pl_host_ctx.h"

namespace {

int check_quant_params(const pngloss_hip_quant_params2 *params)
{
    if (!params || params->max_colors < PLQ_MIN_COLORS || params->max_colors > PLQ_MAX_COLORS || params->rounds > PLQ_MAX_ROUNDS) return PNGLOSS_INVALID_ARGUMENT;
    if (params->dither > PNGLOSS_HIP_DITHER_FLOYD_STEINBERG || params->reserved) return PNGLOSS_INVALID_ARGUMENT;
    return PNGLOSS_SUCCESS;
}

/* the old record as the new one: no dithering */
const pngloss_hip_quant_params2 *widen(const pngloss_hip_quant_params *params, pngloss_hip_quant_params2 &wide)
{
    if (!params) return nullptr;
    wide = pngloss_hip_quant_params2{ params->max_colors, params->rounds, PNGLOSS_HIP_DITHER_NONE, 0 };
    return &wide;
}

template <class Image> int check_quant_sizes(const Image *images, size_t n, const void *const *pixels_of)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t px = (uint64_t)images[i].width * images[i].height;
        if (px && !pixels_of[i]) return PNGLOSS_INVALID_ARGUMENT;
        if (!plq_pixels_ok(px)) return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_SUCCESS;
}

PlQuantLayout quant_layout_of(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs)
{
    return pl_quant_layout(width, height, inputs, sizeof(PlIndexJob), sizeof(PlQuantJob), sizeof(PlDistortJob), sizeof(PliRecord), sizeof(PlDistortRecord));
}

/* the whole workspace of a call: the quantiser's, and behind it -- when the call dithers -- the dither pass's job table and error lines */
struct QuantWorkspace {
    PlQuantLayout lay;
    PlDitherLayout dither;
    bool dithers = false;
    size_t total() const { return dithers ? dither.total : lay.total; }
};
QuantWorkspace quant_workspace_of(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs, const pngloss_hip_quant_params2 &params)
{
    QuantWorkspace ws;
    ws.lay = quant_layout_of(width, height, inputs);
    ws.dithers = params.dither == PNGLOSS_HIP_DITHER_FLOYD_STEINBERG;
    if (ws.dithers) ws.dither = pl_dither_layout(width, ws.lay.total, sizeof(PlDitherJob));
    return ws;
}

/* The images img[0 .. n) (device, width[i] * height[i] words each) quantised in place, in the workspace ctx->d_quant, which the caller has grown to
 * ws.total().  Waits for `stream` twice: behind the colour counts and the histograms, and at the end. */
int quantize_on(pngloss_hip_ctx *ctx, const QuantWorkspace &ws, const std::vector<uint32_t *> &img, const std::vector<uint32_t> &width,
                const std::vector<uint32_t> &height, const pngloss_hip_quant_params2 &params, pngloss_hip_quant_report *reports, hipStream_t stream)
{
    const PlQuantLayout &lay = ws.lay;
    const size_t n = img.size();
    char *const base = ctx->d_quant.p;
    uint32_t *const d_counts = reinterpret_cast<uint32_t *>(base + lay.counts);
    PliRecord *const d_records = reinterpret_cast<PliRecord *>(base + lay.records);
    PlDistortRecord *const d_distort = reinterpret_cast<PlDistortRecord *>(base + lay.distort_records);
    std::vector<size_t> live;                       /* the images with pixels: entry k of every job table is image live[k] */
    std::vector<PlIndexJob> ijobs;
    std::vector<PlQuantJob> qjobs;
    uint64_t max_pixels = 0;
    for (size_t i = 0; i < n; i++) {
        reports[i] = pngloss_hip_quant_report{};
        reports[i].exact = 1;                       /* (an image without pixels: exact, no entries) */
        const uint64_t px = (uint64_t)width[i] * height[i];
        if (!px) continue;
        const PlQuantImage &m = lay.im[i];
        live.push_back(i);
        ijobs.push_back(PlIndexJob{ img[i], px, width[i], height[i], reinterpret_cast<uint64_t *>(base + m.table), d_counts + i, d_records + i, nullptr, nullptr, 0, 0 });
        qjobs.push_back(PlQuantJob{ img[i], reinterpret_cast<uint32_t *>(base + m.out), px, reinterpret_cast<uint32_t *>(base + m.hist),
                                    reinterpret_cast<uint32_t *>(base + m.pal), reinterpret_cast<uint64_t *>(base + m.acc), 0, 0 });
        max_pixels = std::max(max_pixels, px);
    }
    if (live.empty()) return PNGLOSS_SUCCESS;
    const PlIndexJob *const d_ijobs = reinterpret_cast<const PlIndexJob *>(base + lay.index_jobs);
    const PlQuantJob *const d_qjobs = reinterpret_cast<const PlQuantJob *>(base + lay.quant_jobs);
    const PlDistortJob *const d_djobs = reinterpret_cast<const PlDistortJob *>(base + lay.distort_jobs);

    /* the colours and the histogram of every image; the one synchronisation the median cut needs */
    std::vector<uint32_t> counts(n, 0), hists(live.size() * (size_t)PLQ_BINS);
    PL_CHECK(hipMemsetAsync(base + lay.counts, 0, lay.zeroed, stream));
    PL_CHECK(hipMemsetAsync(base + lay.tables, 0xFF, lay.tables_bytes, stream));
    PL_CHECK(hipMemsetAsync(base + lay.hists, 0, lay.hists_bytes, stream));
    PL_CHECK(hipMemcpyAsync(base + lay.index_jobs, ijobs.data(), sizeof(PlIndexJob) * ijobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(hipMemcpyAsync(base + lay.quant_jobs, qjobs.data(), sizeof(PlQuantJob) * qjobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(pl_launch_index_count(d_ijobs, ijobs.size(), max_pixels, stream));
    PL_CHECK(pl_launch_quant_hist(d_qjobs, qjobs.size(), max_pixels, stream));
    PL_CHECK(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
    for (size_t k = 0; k < live.size(); k++)
        PL_CHECK(hipMemcpyAsync(hists.data() + k * (size_t)PLQ_BINS, qjobs[k].hist, PLL_QUANT_HIST, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));

    /* exact images leave here; the others get their initial palette */
    std::vector<PlQuantJob> work;
    std::vector<PlDitherJob> dither;
    std::vector<PlDistortJob> djobs(live.size());
    std::vector<uint32_t> pals(n * (size_t)PLQ_MAX_COLORS, 0);
    uint64_t work_pixels = 0;
    for (size_t k = 0; k < live.size(); k++) {
        const size_t i = live[k];
        reports[i].colors_in = pli_colors_of(counts[i]);
        reports[i].exact = reports[i].colors_in <= params.max_colors;
        djobs[k] = PlDistortJob{ img[i], reports[i].exact ? img[i] : qjobs[k].out, qjobs[k].pixels, d_distort + i };
        if (reports[i].exact) continue;
        const std::vector<uint32_t> first = plq_median_cut(hists.data() + k * (size_t)PLQ_BINS, params.max_colors);
        if (first.empty() || first.size() > params.max_colors) {
            std::fprintf(stderr, "pngloss_hip: quantize: image %zu: a histogram without pixels\n", i);
            return PNGLOSS_HIP_ERROR;
        }
        std::copy(first.begin(), first.end(), pals.begin() + (long)(i * (size_t)PLQ_MAX_COLORS));
        qjobs[k].entries = (uint32_t)first.size();
        work.push_back(qjobs[k]);
        if (ws.dithers)
            dither.push_back(PlDitherJob{ img[i], qjobs[k].out, qjobs[k].pal, reinterpret_cast<PlfErr *>(base + ws.dither.line[i]), width[i], height[i], qjobs[k].entries, 0 });
        work_pixels = std::max(work_pixels, qjobs[k].pixels);
    }
    if (!work.empty()) {
        PL_CHECK(hipMemcpyAsync(base + lay.pals, pals.data(), PLL_QUANT_PAL * n, hipMemcpyHostToDevice, stream));
        PL_CHECK(hipMemcpyAsync(base + lay.quant_jobs, work.data(), sizeof(PlQuantJob) * work.size(), hipMemcpyHostToDevice, stream));   /* (the histogram kernel has read its table: synchronised above) */
        for (uint32_t round = 0; round < params.rounds; round++) {
            PL_CHECK(pl_launch_quant_assign(d_qjobs, work.size(), work_pixels, stream));
            PL_CHECK(pl_launch_quant_update(d_qjobs, work.size(), stream));
        }
        if (ws.dithers) {
            PL_CHECK(hipMemcpyAsync(base + ws.dither.jobs, dither.data(), sizeof(PlDitherJob) * dither.size(), hipMemcpyHostToDevice, stream));
            PL_CHECK(pl_launch_dither(reinterpret_cast<const PlDitherJob *>(base + ws.dither.jobs), dither.size(), stream));
        } else {
            PL_CHECK(pl_launch_quant_remap(d_qjobs, work.size(), work_pixels, stream));
        }
    }
    /* the record of (input, output) while both exist, then the output over the input */
    PL_CHECK(hipMemcpyAsync(base + lay.distort_jobs, djobs.data(), sizeof(PlDistortJob) * djobs.size(), hipMemcpyHostToDevice, stream));
    PL_CHECK(pl_launch_distort(d_djobs, djobs.size(), max_pixels, stream));
    for (const PlQuantJob &j : work)
        PL_CHECK(hipMemcpyAsync(const_cast<uint32_t *>(j.img), j.out, (size_t)j.pixels * 4, hipMemcpyDeviceToDevice, stream));
    /* the palette that is reported: the colours of the image as it is now, counted and ordered by the indexed side's own kernels */
    PL_CHECK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * n, stream));
    PL_CHECK(hipMemsetAsync(base + lay.tables, 0xFF, lay.tables_bytes, stream));
    PL_CHECK(pl_launch_index_count(d_ijobs, ijobs.size(), max_pixels, stream));
    PL_CHECK(pl_launch_index_palette(d_ijobs, ijobs.size(), stream));
    std::vector<PliRecord> records(n);
    std::vector<PlDistortRecord> distort(n);
    PL_CHECK(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(records.data(), d_records, sizeof(PliRecord) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(distort.data(), d_distort, sizeof(PlDistortRecord) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    for (size_t i : live) {
        pngloss_hip_quant_report &rep = reports[i];
        if (records[i].entries != counts[i] || counts[i] < 1 || counts[i] > params.max_colors) {
            std::fprintf(stderr, "pngloss_hip: quantize: image %zu has %u colours in its table, its counter says %u, %u were allowed\n", i, records[i].entries, counts[i], params.max_colors);
            return PNGLOSS_HIP_ERROR;
        }
        rep.entries = records[i].entries;
        std::copy(records[i].words, records[i].words + rep.entries, rep.palette);
        std::memcpy(&rep.distortion, &distort[i], sizeof rep.distortion);
    }
    return PNGLOSS_SUCCESS;
}

/* the share of one context in the host form: its images up into the workspace, quantised there, the changed ones back */
int quantize_host_share(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 &params, pngloss_hip_quant_report *reports)
{
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    const QuantWorkspace ws = quant_workspace_of(width, height, true, params);
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

/* both forms of pngloss_hip_quantize_batch */
int quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
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
    const QuantWorkspace ws = quant_workspace_of(width, height, false, *params);
    const int rc = ctx->d_quant.grow(ws.total(), 8);
    if (rc) return rc;
    std::vector<uint32_t *> img(n);
    for (size_t i = 0; i < n; i++) img[i] = static_cast<uint32_t *>(images[i].d_rgba);
    return quantize_on(ctx, ws, img, width, height, *params, reports, static_cast<hipStream_t>(stream_));
}

/* both forms of pngloss_hip_multi_quantize_batch_host */
int multi_quantize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params,
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
        const int rc = quantize_host_share(ctx, mine.images.data(), mine.n(), *params, own.data());
        for (size_t k = 0; k < mine.n(); k++) reports[mine.who[k]] = own[k];
        return rc;
    });
}

} // namespace

extern "C" {

int pngloss_hip_quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params *params,
                               pngloss_hip_quant_report *reports, void *stream)
{
    pngloss_hip_quant_params2 wide;
    return quantize_batch(ctx, images, n, widen(params, wide), reports, stream);
}

int pngloss_hip_multi_quantize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params *params,
                                          pngloss_hip_quant_report *reports)
{
    pngloss_hip_quant_params2 wide;
    return multi_quantize_batch_host(m, images, n, widen(params, wide), reports);
}

int pngloss_hip_quantize_batch2(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
                                pngloss_hip_quant_report *reports, void *stream)
{
    return quantize_batch(ctx, images, n, params, reports, stream);
}

int pngloss_hip_multi_quantize_batch_host2(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params,
                                           pngloss_hip_quant_report *reports)
{
    return multi_quantize_batch_host(m, images, n, params, reports);
}

} /* extern "C" */

/*
 * pl_host_measure.hip -- the host side of the two measuring kernels (pl_distort, pl_ssim): their job tables, as enqueue and the searches upload
 * them, and the stand-alone comparisons (pl_host_ctx.h has the map of the host files).
 */
#include "pl_host_ctx.h"

/* One table of distortion jobs, as pl_distort (and pl_keep) want it: image i is `pixels[i]` words at img[i], compared with the original at keep[i];
 * jobs[i].record = d_records + i. */
void fill_distort_jobs(PlDistortJob *jobs, PlDistortRecord *d_records, size_t n, const void *const *img, const void *const *keep, const uint64_t *pixels)
{
    for (size_t i = 0; i < n; i++) {
        jobs[i].keep = static_cast<uint32_t *>(const_cast<void *>(keep[i]));
        jobs[i].img = static_cast<const uint32_t *>(img[i]);
        jobs[i].pixels = pixels[i];
        jobs[i].record = d_records + i;
    }
}

/* The job table of a measurement into the keep arena (which the caller has grown to lay.total), its records zeroed: image i is `pixels[i]` words at img[i],
 * compared with the original at keep[i] -- or, keep == nullptr, with the place the layout gives it in the arena, for pl_keep to fill. */
int upload_distort_jobs(pngloss_hip_ctx *ctx, const PlKeepLayout &lay, size_t n, const void *const *img, const void *const *keep, const uint64_t *pixels, hipStream_t stream)
{
    PlDistortRecord *const d_rec = reinterpret_cast<PlDistortRecord *>(ctx->d_keep.p + lay.records);
    std::vector<const void *> own(keep ? 0 : n);
    for (size_t i = 0; i < own.size(); i++) own[i] = ctx->d_keep.p + lay.image[i];
    ctx->h_dj.assign(n, PlDistortJob{});
    fill_distort_jobs(ctx->h_dj.data(), d_rec, n, img, keep ? keep : own.data(), pixels);
    PL_CHECK(hipMemcpyAsync(ctx->d_keep.p + lay.jobs, ctx->h_dj.data(), sizeof(PlDistortJob) * n, hipMemcpyHostToDevice, stream));
    PL_CHECK(hipMemsetAsync(d_rec, 0, sizeof(PlDistortRecord) * n, stream));
    return PNGLOSS_SUCCESS;
}

/* One table of SSIM jobs and their records, as pl_ssim wants them before its launch: pair i is the width[i] x height[i] image b[i] against the
 * original a[i]; jobs[i].record = d_records + i, records[i] = the record with no window added yet (visible: as pl_ssim_visible wants it).  Returns the largest tile count (sizes the grid). */
uint64_t fill_ssim_jobs(PlSsimJob *jobs, PlSsimRecord *records, PlSsimRecord *d_records, size_t n, const void *const *a, const void *const *b,
                        const uint32_t *width, const uint32_t *height, bool visible)
{
    uint64_t max_tiles = 0;
    for (size_t i = 0; i < n; i++) {
        jobs[i] = PlSsimJob{ static_cast<const uint32_t *>(a[i]), static_cast<const uint32_t *>(b[i]), width[i], height[i], d_records + i };
        records[i] = visible ? pls_record_begin_visible() : pls_record_begin(width[i], height[i]);
        max_tiles = std::max(max_tiles, pls_geom(width[i], height[i]).tiles);
    }
    return max_tiles;
}

/* The same into the context's SSIM buffer (grown here: call it before anything of the batch is enqueued), uploaded on `stream` */
int upload_ssim_jobs(pngloss_hip_ctx *ctx, size_t n, const void *const *a, const void *const *b, const uint32_t *width, const uint32_t *height,
                     hipStream_t stream, PlSsimLayout &lay, uint64_t &max_tiles, bool visible)
{
    lay = pl_ssim_layout(n, sizeof(PlSsimJob), sizeof(PlSsimRecord));
    const int rc = ctx->d_ssim.grow(lay.total, 8);
    if (rc) return rc;
    ctx->h_ssj.assign(n, PlSsimJob{});
    ctx->h_ssr.assign(n, PlSsimRecord{});
    max_tiles = fill_ssim_jobs(ctx->h_ssj.data(), ctx->h_ssr.data(), reinterpret_cast<PlSsimRecord *>(ctx->d_ssim.p + lay.records), n, a, b, width, height, visible);
    PL_CHECK(hipMemcpyAsync(ctx->d_ssim.p + lay.jobs, ctx->h_ssj.data(), sizeof(PlSsimJob) * n, hipMemcpyHostToDevice, stream));
    PL_CHECK(hipMemcpyAsync(ctx->d_ssim.p + lay.records, ctx->h_ssr.data(), sizeof(PlSsimRecord) * n, hipMemcpyHostToDevice, stream));
    return PNGLOSS_SUCCESS;
}

/* the three stand-alone measurements: one launch of pl_distort / pl_ssim (visible: of their visible forms) on the caller's pairs */
static int compare_distortion(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out, hipStream_t stream, bool visible)
{
    std::vector<const void *> a(n), b(n);
    std::vector<uint64_t> pixels(n);
    uint64_t max_pixels = 0;
    for (size_t i = 0; i < n; i++) {
        pixels[i] = (uint64_t)pairs[i].width * pairs[i].height;
        if (pixels[i] && (!pairs[i].d_a || !pairs[i].d_b)) return PNGLOSS_INVALID_ARGUMENT;
        a[i] = pairs[i].d_a; b[i] = pairs[i].d_b;
        max_pixels = std::max(max_pixels, pixels[i]);
    }
    PL_CHECK(hipSetDevice(ctx->device));
    const PlKeepLayout lay = pl_keep_layout(std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0), false, sizeof(PlDistortJob), sizeof(PlDistortRecord));
    int rc = ctx->d_keep.grow(lay.total, 8);
    if (rc) return rc;
    rc = upload_distort_jobs(ctx, lay, n, b.data(), a.data(), pixels.data(), stream);
    if (rc) return rc;
    PL_CHECK(pl_launch_distort(reinterpret_cast<const PlDistortJob *>(ctx->d_keep.p + lay.jobs), n, max_pixels, stream, visible));
    PL_CHECK(hipMemcpyAsync(out, ctx->d_keep.p + lay.records, sizeof(pngloss_hip_distortion) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    return PNGLOSS_SUCCESS;
}

static int compare_ssim(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_ssim *out, hipStream_t stream, bool visible)
{
    std::vector<const void *> a(n), b(n);
    std::vector<uint32_t> width, height;
    batch_dims(pairs, n, width, height);
    for (size_t i = 0; i < n; i++) {
        if (pairs[i].width && pairs[i].height && (!pairs[i].d_a || !pairs[i].d_b)) return PNGLOSS_INVALID_ARGUMENT;
        a[i] = pairs[i].d_a; b[i] = pairs[i].d_b;
    }
    PL_CHECK(hipSetDevice(ctx->device));
    PlSsimLayout lay;
    uint64_t max_tiles = 0;
    const int rc = upload_ssim_jobs(ctx, n, a.data(), b.data(), width.data(), height.data(), stream, lay, max_tiles, visible);
    if (rc) return rc;
    PL_CHECK(pl_launch_ssim(reinterpret_cast<const PlSsimJob *>(ctx->d_ssim.p + lay.jobs), n, max_tiles, stream, visible));
    PL_CHECK(hipMemcpyAsync(out, ctx->d_ssim.p + lay.records, sizeof(pngloss_hip_ssim) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    return PNGLOSS_SUCCESS;
}

extern "C" {

int pngloss_hip_compare_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out, void *stream_)
{
    if (!ctx || (n && (!pairs || !out))) return PNGLOSS_INVALID_ARGUMENT;
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    return compare_distortion(ctx, pairs, n, out, static_cast<hipStream_t>(stream_), false);
}

int pngloss_hip_compare_batch_ssim(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_ssim *out, void *stream_)
{
    if (!ctx || (n && (!pairs || !out))) return PNGLOSS_INVALID_ARGUMENT;
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    return compare_ssim(ctx, pairs, n, out, static_cast<hipStream_t>(stream_), false);
}

int pngloss_hip_compare_batch_visible(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out_distortion,
                                      pngloss_hip_ssim *out_ssim, void *stream_)
{
    if (!ctx || (n && !pairs)) return PNGLOSS_INVALID_ARGUMENT;
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    int rc = out_distortion ? compare_distortion(ctx, pairs, n, out_distortion, static_cast<hipStream_t>(stream_), true) : PNGLOSS_SUCCESS;
    if (rc == PNGLOSS_SUCCESS && out_ssim) rc = compare_ssim(ctx, pairs, n, out_ssim, static_cast<hipStream_t>(stream_), true);
    return rc;
}

double pngloss_hip_ssim_mean(const pngloss_hip_ssim *r, unsigned channel_mask)
{
    return r ? pls_mean(r->windows, r->sum_q16, channel_mask) : std::nan("");
}

double pngloss_hip_psnr_db(const pngloss_hip_distortion *d, unsigned channel_mask)
{
    return d ? pld_psnr_db(d->pixels, d->sq_err, channel_mask) : std::nan("");
}

} /* extern "C" */

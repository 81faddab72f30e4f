/*
 * pl_host_quant_target.hip -- the colour count of the quantiser searched per image from a distortion target (include/pngloss_hip_quant_target.h;
 * pl_host_ctx.h has the map of the host files).  What the search DECIDES is pl_colors.h's; the stages it runs are pl_host_quant.hip's:
 *   once per call   quant_survey: the colour counts and the histograms, one synchronisation; the histograms stay on the host
 *   per round       every image still searching gets the median cut at its own next N (the cut's state after k splits does not depend on where it
 *                   stops: this is the palette pngloss_hip_quantize_batch2 at that N starts from); ONE job table with a different `entries` per job,
 *                   the rounds over it (quant_refine), then the measuring pass -- pl_quant_measure, which stores no pixel; with dithering pl_dither
 *                   into `out` and pl_distort --, one download of the records and of the final palettes, one synchronisation
 *   the close       quant_close over the palettes the search kept: the tail of every quantiser call, so `quant` is by construction that call's report
 * The state of the search is palettes, not images: the host keeps the final palette of the last accepted probe, which is the one the procedure
 * ends on.
 * In the premultiplied space (include/pngloss_hip_quant_space.h; ws.visible) a probe's record is the visible-mode one: the measuring kernels count
 * `pixels` themselves, a record without visible pixels is accepted, and an exact probe -- which needs no device work and passes whatever it counts --
 * takes its `pixels` from the record of the close.
 */
#include "pl_host_ctx.h"

namespace {

/* what the search keeps of the probe an image will end on */
struct Kept {
    uint32_t colors = 0, entries = 0;
    PlDistortRecord record = {};
};

int quantize_target_on(pngloss_hip_ctx *ctx, const QuantWorkspace &ws, const std::vector<uint32_t *> &img, const std::vector<uint32_t> &width,
                       const std::vector<uint32_t> &height, const pngloss_hip_quant_params2 &params, const pngloss_hip_quant_target &target,
                       pngloss_hip_quant_target_report *reports, hipStream_t stream)
{
    const size_t n = img.size();
    const PlQuantLayout &lay = ws.lay;
    QuantBatch b{ ctx, ws, img, width, height, stream };
    std::vector<pngloss_hip_quant_report> quant(n);
    int rc = quant_survey(b, quant.data());
    if (rc) return rc;
    char *const base = b.base();
    PlDistortRecord *const d_distort = reinterpret_cast<PlDistortRecord *>(base + lay.distort_records);

    std::vector<PlColorsSearch> search(n, pl_colors_begin(params.max_colors));
    std::vector<uint64_t> pixels(n);
    std::vector<size_t> k_of(n, 0);                 /* image -> its entry in the batch's job tables */
    for (size_t k = 0; k < b.live.size(); k++) k_of[b.live[k]] = k;
    std::vector<Kept> kept(n);
    std::vector<uint32_t> pals(n * (size_t)PLQ_MAX_COLORS, 0), kept_pals(n * (size_t)PLQ_MAX_COLORS, 0);
    std::vector<uint32_t> in_out(n, 0);             /* with dithering: the N whose result lies in the image's `out`; 0: none */
    auto pal_of = [](std::vector<uint32_t> &p, size_t i) { return p.begin() + (long)(i * (size_t)PLQ_MAX_COLORS); };
    /* the verdict of a probe that ran on the device, or of one that needed none (an exact one: all zero apart from `pixels`) */
    auto take = [&](size_t i, const PlDistortRecord &rec, uint32_t entries) {
        const uint32_t colors = search[i].next;
        const bool ends_here = search[i].first;     /* a refused first probe is the image's result all the same */
        const bool accepted = pl_colors_accept(target, rec);       /* (a record with pixels == 0 -- nothing visible in either image -- passes there) */
        if (accepted || ends_here) {
            kept[i] = Kept{ colors, entries, rec };
            std::copy(pal_of(pals, i), pal_of(pals, i) + PLQ_MAX_COLORS, pal_of(kept_pals, i));
        }
        pl_colors_step(search[i], accepted);
    };
    for (size_t i = 0; i < n; i++) pixels[i] = (uint64_t)width[i] * height[i];

    for (;;) {
        /* the probes that need no device work */
        for (size_t i = 0; i < n; i++)
            while (!search[i].done && pl_colors_probe_is_exact(pixels[i], quant[i].colors_in, search[i].next)) {
                PlDistortRecord zero = {};
                zero.pixels = pixels[i];
                take(i, zero, 0);
            }
        const std::vector<std::pair<uint32_t, uint32_t>> round = pl_colors_round(search);
        if (round.empty()) break;
        std::vector<size_t> work;
        for (const auto &probe : round) {
            const size_t k = k_of[probe.first];
            rc = quant_first_palette(b, k, probe.second, pals);
            if (rc) return rc;
            work.push_back(k);
        }
        std::vector<PlQuantJob> jobs;
        uint64_t work_pixels = 0;
        PL_CHECK(hipMemsetAsync(d_distort, 0, sizeof(PlDistortRecord) * n, stream));
        rc = quant_refine(b, work, pals, params.rounds, jobs, work_pixels);
        if (rc) return rc;
        /* record k of the round is job k's.  (Not in the last assign pass: that one searches the palette BEFORE the last update.) */
        std::vector<PlDistortJob> djobs;
        if (ws.dithers) {
            rc = quant_dither(b, work);
            if (rc) return rc;
            for (size_t r = 0; r < work.size(); r++) {
                djobs.push_back(PlDistortJob{ const_cast<uint32_t *>(jobs[r].img), jobs[r].out, jobs[r].pixels, d_distort + r });
                in_out[round[r].first] = round[r].second;
            }
            PL_CHECK(hipMemcpyAsync(base + lay.distort_jobs, djobs.data(), sizeof(PlDistortJob) * djobs.size(), hipMemcpyHostToDevice, stream));
            PL_CHECK(pl_launch_distort(reinterpret_cast<const PlDistortJob *>(base + lay.distort_jobs), djobs.size(), work_pixels, stream, ws.visible));
        } else {
            PL_CHECK(pl_launch_quant_measure(b.d_qjobs(), d_distort, jobs.size(), work_pixels, stream, ws.visible));
        }
        std::vector<PlDistortRecord> records(work.size());
        PL_CHECK(hipMemcpyAsync(records.data(), d_distort, sizeof(PlDistortRecord) * records.size(), hipMemcpyDeviceToHost, stream));
        PL_CHECK(hipMemcpyAsync(pals.data(), base + lay.pals, PLL_QUANT_PAL * n, hipMemcpyDeviceToHost, stream));
        PL_CHECK(hipStreamSynchronize(stream));
        for (size_t r = 0; r < work.size(); r++) {
            if (!ws.visible) records[r].pixels = jobs[r].pixels;
            take(round[r].first, records[r], jobs[r].entries);
        }
    }

    /* the close: the kept palettes up, the pass into `out` for every image that is not exact at its N (with dithering: unless that result lies there) */
    std::vector<size_t> work, pass;
    std::vector<uint32_t> allowed(n, params.max_colors);
    for (size_t i = 0; i < n; i++) {
        allowed[i] = search[i].chosen;
        if (!pixels[i]) continue;
        quant[i].exact = quant[i].colors_in <= search[i].chosen;
        if (quant[i].exact) continue;
        if (kept[i].colors != search[i].chosen || !kept[i].entries) {
            std::fprintf(stderr, "pngloss_hip: quantize target: image %zu ends on %u colours, the palette kept is that of %u\n", i, search[i].chosen, kept[i].colors);
            return PNGLOSS_HIP_ERROR;
        }
        b.qjobs[k_of[i]].entries = kept[i].entries;
        work.push_back(k_of[i]);
        if (!ws.dithers || in_out[i] != search[i].chosen) pass.push_back(k_of[i]);
    }
    std::vector<PlQuantJob> jobs;
    uint64_t work_pixels = 0;
    PL_CHECK(hipMemsetAsync(d_distort, 0, sizeof(PlDistortRecord) * n, stream));
    rc = quant_refine(b, work, kept_pals, 0, jobs, work_pixels);
    if (rc) return rc;
    rc = quant_close(b, jobs, work_pixels, pass, allowed, quant.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
        pngloss_hip_quant_target_report &rep = reports[i];
        rep = pngloss_hip_quant_target_report{};
        rep.colors = search[i].chosen;
        rep.reached = search[i].reached ? 1u : 0u;
        rep.probes = search[i].probes;
        rep.accepted_mask = search[i].accepted_mask;
        std::copy(search[i].probed, search[i].probed + PLC_MAX_PROBES, rep.probed);
        std::memcpy(&rep.probe_distortion, &kept[i].record, sizeof rep.probe_distortion);
        rep.quant = quant[i];
        if (ws.visible && quant[i].exact) rep.probe_distortion.pixels = quant[i].distortion.pixels;
        if (!ws.dithers && std::memcmp(&rep.probe_distortion, &rep.quant.distortion, sizeof rep.probe_distortion) != 0) {
            std::fprintf(stderr, "pngloss_hip: quantize target: image %zu: the probe at %u colours measured another record than the result has\n", i, rep.colors);
            return PNGLOSS_HIP_ERROR;
        }
    }
    return PNGLOSS_SUCCESS;
}

/* the share of one context in the host form: its images up into the workspace, searched there, the changed ones back */
int quantize_target_host_share(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 &params,
                               uint32_t space, const pngloss_hip_quant_target &target, pngloss_hip_quant_target_report *reports)
{
    if (batch_in_flight_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    const QuantWorkspace ws = quant_workspace_of(width, height, true, params, space);
    int rc = ctx->d_quant.grow(ws.total(), 8);
    if (rc == PNGLOSS_SUCCESS) rc = ensure_copy_stream(ctx);
    if (rc) return rc;
    hipStream_t stream = ctx->copy_stream;
    std::vector<uint32_t *> img(n);
    for (size_t i = 0; i < n; i++) {
        const size_t bytes = (size_t)width[i] * height[i] * 4;
        img[i] = reinterpret_cast<uint32_t *>(ctx->d_quant.p + ws.lay.im[i].in);
        if (bytes) PL_CHECK(hipMemcpyAsync(img[i], images[i].rgba, bytes, hipMemcpyHostToDevice, stream));
    }
    rc = quantize_target_on(ctx, ws, img, width, height, params, target, reports, stream);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
        const size_t bytes = (size_t)width[i] * height[i] * 4;
        if (bytes && !reports[i].quant.exact) PL_CHECK(hipMemcpyAsync(images[i].rgba, img[i], bytes, hipMemcpyDeviceToHost, stream));
    }
    PL_CHECK(hipStreamSynchronize(stream));
    return PNGLOSS_SUCCESS;
}

/* the checks both forms make, all before any device work */
template <class Image, class Pixels>
int check_target_call(const void *object, const Image *images, size_t n, const pngloss_hip_quant_params2 *params, const pngloss_hip_quant_target *target,
                      const void *reports, Pixels pixels_at)
{
    if (!object || (n && (!images || !reports)) || check_quant_params(params) || pl_colors_target_check(target)) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<const void *> pixels_of(n);
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    for (size_t i = 0; i < n; i++) pixels_of[i] = pixels_at(images[i]);
    return check_quant_pixels(width.data(), height.data(), n, pixels_of.data());
}

} // namespace

/* every form of pngloss_hip_quantize_batch_target; space: PNGLOSS_HIP_QUANT_SPACE_*, checked by the caller */
int quantize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                          const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream_)
{
    if (check_target_call(ctx, images, n, params, target, reports, [](const pngloss_hip_image_desc &im) { return (const void *)im.d_rgba; })) return PNGLOSS_INVALID_ARGUMENT;
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
    return quantize_target_on(ctx, ws, img, width, height, *params, *target, reports, static_cast<hipStream_t>(stream_));
}

/* every form of pngloss_hip_multi_quantize_batch_host_target */
int multi_quantize_batch_host_target(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                                     const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports)
{
    if (check_target_call(m, images, n, params, target, reports, [](const pngloss_hip_host_image &im) { return (const void *)im.rgba; })) return PNGLOSS_INVALID_ARGUMENT;
    if (m->ctx.empty()) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    return deal_over_contexts(m, images, n, nullptr, nullptr, nullptr, false, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        std::vector<pngloss_hip_quant_target_report> own(mine.n());
        const int rc = quantize_target_host_share(ctx, mine.images.data(), mine.n(), *params, space, *target, own.data());
        for (size_t k = 0; k < mine.n(); k++) reports[mine.who[k]] = own[k];
        return rc;
    });
}

extern "C" {

int pngloss_hip_quantize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
                                      const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream)
{
    return quantize_batch_target(ctx, images, n, params, PNGLOSS_HIP_QUANT_SPACE_RGBA, target, reports, stream);
}

int pngloss_hip_multi_quantize_batch_host_target(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params,
                                                 const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports)
{
    return multi_quantize_batch_host_target(m, images, n, params, PNGLOSS_HIP_QUANT_SPACE_RGBA, target, reports);
}

} /* extern "C" */

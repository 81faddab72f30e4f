/*
 * pl_host_search.hip -- a strength per image, searched (pl_host_ctx.h has the map of the host files): pl_target.h and pl_size.h have the two rules,
 * pl_search.h decides what is kept and which arena regions are copied where, and this does what they say (include/pngloss_hip.h has the contracts).
 */
#include "pl_host_ctx.h"

namespace {
/* What both searches do on the device: region moves, batches and distortion measurements on the search arena (ctx->d_target, laid out as `lay`).  The host
 * tables stay alive until the call's last synchronisation: asynchronous copies read them. */
struct SearchDevice {
    pngloss_hip_ctx *ctx;
    const pngloss_hip_image_desc *images;
    const PlTargetLayout &lay;
    long bleed;
    hipStream_t stream;
    std::vector<std::vector<PlMoveJob>> move_tables;
    std::vector<std::vector<PlDistortJob>> distort_tables;

    char *at(size_t offset) const { return ctx->d_target.p + offset; }
    void *address(uint32_t i, PlArenaRegion r) const
    {
        const PlTargetImage &m = lay.image[i];
        switch (r) {
        case PLA_IMAGE: return images[i].d_rgba;
        case PLA_FILTERS: return images[i].d_row_filters;
        case PLA_ORIG: return at(m.orig);
        case PLA_BEST: return at(m.best);
        case PLA_BEST_FILTERS: return at(m.best_filters);
        case PLA_ROWS: return at(m.rows);
        case PLA_IDS: return at(m.ids);
        case PLA_BEST_ROWS: return at(m.best_rows);
        case PLA_BEST_IDS: return at(m.best_ids);
        default: return nullptr;
        }
    }
    /* one launch of pl_move for a table of jobs */
    int move(std::vector<PlMoveJob> jobs)
    {
        if (jobs.empty()) return PNGLOSS_SUCCESS;
        uint64_t max_bytes = 0;
        for (const PlMoveJob &j : jobs) max_bytes = std::max(max_bytes, j.bytes);
        move_tables.push_back(std::move(jobs));
        const std::vector<PlMoveJob> &tb = move_tables.back();
        PlMoveJob *const d_moves = reinterpret_cast<PlMoveJob *>(at(lay.moves));
        PL_CHECK(hipMemcpyAsync(d_moves, tb.data(), sizeof(PlMoveJob) * tb.size(), hipMemcpyHostToDevice, stream));
        PL_CHECK(pl_launch_move(d_moves, tb.size(), max_bytes, stream));
        return PNGLOSS_SUCCESS;
    }
    /* ... for the moves pl_search.h asks for: each with its addresses and its bytes; one of 0 bytes is no job */
    int move(const std::vector<PlSearchMove> &moves)
    {
        std::vector<PlMoveJob> jobs;
        for (const PlSearchMove &m : moves) {
            const pngloss_hip_image_desc &im = images[m.image];
            const uint64_t bytes = pl_search_region_bytes(m.src, im.width, im.height, im.d_row_filters != nullptr, lay.image[m.image].pitch);
            if (bytes) jobs.push_back(PlMoveJob{ address(m.image, m.src), address(m.image, m.dst), bytes });
        }
        return move(std::move(jobs));
    }
    /* one ordinary batch: the images `who` at `strength`, as the synchronous call asks for it, with nothing measured behind it (the search measures against its
     * own originals: the keep arena is laid out afresh by every enqueue).  emits: nullptr, or where each one's scanlines go */
    int run(uint32_t strength, const std::vector<uint32_t> &who, const EmitTarget *emits, std::vector<pngloss_hip_result> &res)
    {
        std::vector<pngloss_hip_image_desc> descs(who.size());
        res.assign(who.size(), pngloss_hip_result{});
        for (size_t k = 0; k < who.size(); k++) descs[k] = images[who[k]];
        BatchCall call{ strength, bleed, stream, Measure{} };
        call.sync_call = call.three_groups_ok = true; call.emits = emits;
        int rc = enqueue(ctx, descs.data(), descs.size(), call);
        if (rc == PNGLOSS_SUCCESS) rc = finish(ctx, res.data(), res.size());
        return pl_rc_is_hard(rc) ? rc : PNGLOSS_SUCCESS;           /* (single images that failed say so in their status) */
    }
    /* one launch of pl_distort: the images `who` against the search's own originals, the records on their way into got[0 .. who.size()) -- the caller
     * synchronises */
    int distort(const std::vector<uint32_t> &who, bool visible, pngloss_hip_distortion *got)
    {
        distort_tables.emplace_back(who.size());
        std::vector<PlDistortJob> &dj = distort_tables.back();
        PlDistortJob *const d_dj = reinterpret_cast<PlDistortJob *>(at(lay.jobs));
        PlDistortRecord *const d_rec = reinterpret_cast<PlDistortRecord *>(at(lay.records));
        std::vector<const void *> img(who.size()), orig(who.size());
        std::vector<uint64_t> pixels(who.size());
        uint64_t max_pixels = 0;
        for (size_t k = 0; k < who.size(); k++) {
            const size_t i = who[k];
            orig[k] = at(lay.image[i].orig);
            img[k] = images[i].d_rgba;
            pixels[k] = (uint64_t)images[i].width * images[i].height;
            max_pixels = std::max(max_pixels, pixels[k]);
        }
        fill_distort_jobs(dj.data(), d_rec, dj.size(), img.data(), orig.data(), pixels.data());
        PL_CHECK(hipMemcpyAsync(d_dj, dj.data(), sizeof(PlDistortJob) * dj.size(), hipMemcpyHostToDevice, stream));
        PL_CHECK(hipMemsetAsync(d_rec, 0, sizeof(PlDistortRecord) * dj.size(), stream));
        PL_CHECK(pl_launch_distort(d_dj, dj.size(), max_pixels, stream, visible));
        PL_CHECK(hipMemcpyAsync(got, d_rec, sizeof(PlDistortRecord) * dj.size(), hipMemcpyDeviceToHost, stream));
        return PNGLOSS_SUCCESS;
    }
};

/* images: device-resident; the arena (ctx->d_target) has been grown to lay.total.  commit: at the end every image holds the result of its chosen
 * strength (else the images are left as the last probes left them: the host form runs the chosen strengths through the host-window path). */
int target_search(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const PlTargetLayout &lay, const pngloss_hip_target2 &t, bool visible,
                  long bleed, hipStream_t stream, bool commit, pngloss_hip_result *results, pngloss_hip_target_report *reports, pngloss_hip_ssim *ssim_out)
{
    const bool want_ssim = t.min_ssim != 0.0;          /* without the condition the SSIM kernel is never launched; visible: the probes are accepted or refused on records over visible pixels */
    SearchGuard guard{ ctx, false };
    SearchDevice dev{ ctx, images, lay, bleed, stream, {}, {} };
    PlSsimJob *const d_sj = reinterpret_cast<PlSsimJob *>(dev.at(lay.ssim_jobs));
    PlSsimRecord *const d_srec = reinterpret_cast<PlSsimRecord *>(dev.at(lay.ssim_records));
    std::vector<PlTargetTrack> st(n);
    for (size_t i = 0; i < n; i++) st[i].search = pl_target_begin(t.max_strength);
    std::vector<std::vector<PlSsimJob>> ssim_tables;   /* (alive until the last synchronisation, like the tables of `dev`) */
    std::vector<std::vector<PlSsimRecord>> ssim_begins;
    auto run_group = [&](uint32_t strength, const std::vector<uint32_t> &who) -> int {
        std::vector<pngloss_hip_result> res;
        const int rc = dev.run(strength, who, nullptr, res);
        if (rc) return rc;
        for (size_t k = 0; k < who.size(); k++) pl_search_ran(st[who[k]], strength, res[k]);
        return PNGLOSS_SUCCESS;
    };
    /* one launch of pl_distort -- and, with an SSIM condition, one of pl_ssim --: the images `who` against the search's own originals */
    auto measure = [&](const std::vector<uint32_t> &who) -> int {
        if (who.empty()) return PNGLOSS_SUCCESS;
        std::vector<pngloss_hip_distortion> got(who.size());
        const int rc = dev.distort(who, visible, got.data());
        if (rc) return rc;
        std::vector<pngloss_hip_ssim> sgot(want_ssim ? who.size() : 0);
        if (want_ssim) {
            ssim_tables.emplace_back(who.size());
            ssim_begins.emplace_back(who.size());
            std::vector<PlSsimJob> &sj = ssim_tables.back();
            std::vector<const void *> a(who.size()), b(who.size());
            std::vector<uint32_t> w(who.size()), h(who.size());
            for (size_t k = 0; k < who.size(); k++) {
                const size_t i = who[k];
                a[k] = dev.address(who[k], PLA_ORIG); b[k] = images[i].d_rgba;
                w[k] = images[i].width; h[k] = images[i].height;
            }
            const uint64_t max_tiles = fill_ssim_jobs(sj.data(), ssim_begins.back().data(), d_srec, who.size(), a.data(), b.data(), w.data(), h.data(), visible);
            PL_CHECK(hipMemcpyAsync(d_sj, sj.data(), sizeof(PlSsimJob) * sj.size(), hipMemcpyHostToDevice, stream));
            PL_CHECK(hipMemcpyAsync(d_srec, ssim_begins.back().data(), sizeof(PlSsimRecord) * sj.size(), hipMemcpyHostToDevice, stream));
            PL_CHECK(pl_launch_ssim(d_sj, sj.size(), max_tiles, stream, visible));
            PL_CHECK(hipMemcpyAsync(sgot.data(), d_srec, sizeof(PlSsimRecord) * sj.size(), hipMemcpyDeviceToHost, stream));
        }
        PL_CHECK(hipStreamSynchronize(stream));
        for (size_t k = 0; k < who.size(); k++) {
            st[who[k]].last.rec = got[k];
            if (want_ssim) st[who[k]].last.ssim = sgot[k];
        }
        return PNGLOSS_SUCCESS;
    };

    int rc = dev.move(pl_search_open(n));
    if (rc) return rc;
    for (;;) {
        const PlSearchRound round = pl_search_round(st);
        if (round.groups.empty()) break;
        rc = dev.move(round.back);
        for (size_t g = 0; g < round.groups.size() && rc == PNGLOSS_SUCCESS; g++) rc = run_group(round.groups[g].first, round.groups[g].second);      /* one after the other: a context takes one batch at a time */
        if (rc == PNGLOSS_SUCCESS) rc = measure(round.probed);
        if (rc) return rc;
        rc = dev.move(pl_target_settle(st, round.probed, t));
        if (rc) return rc;
    }
    /* the kept results back into the images whose last probe was refused; an image with no accepted probe gets strength 0, run once */
    const PlTargetClose close = pl_target_close(st, commit);
    rc = dev.move(close.fin);
    if (rc == PNGLOSS_SUCCESS && commit && !close.zero.empty()) {
        rc = run_group(0, close.zero);
        if (rc == PNGLOSS_SUCCESS) rc = measure(close.zero);
        pl_target_reran(st, close.zero);
    }
    if (rc) return rc;
    PL_CHECK(hipStreamSynchronize(stream));
    int worst = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < n; i++) {
        const PlTargetTrack &s = st[i];
        if (results) results[i] = s.kept.result;
        if (reports) reports[i] = pngloss_hip_target_report{ s.search.chosen, s.search.probes, s.runs, 0, s.kept.rec };
        if (ssim_out && want_ssim) ssim_out[i] = s.kept.ssim;
        if (s.kept.result.status) worst = PNGLOSS_INTERNAL_ABORT;
    }
    return worst;
}

/* ---- a strength per image from a byte budget: pl_size.h has the rule, pl_search.h the bookkeeping ---- */
/* images: device-resident; the arena (ctx->d_target) has been grown to lay.total, laid out with a scanline region (and, with `streams`, the best
 * result's).  commit: at the end every image holds the result of its chosen strength and `streams` (may be nullptr) are written; else the images are
 * left as the last probes left them (the host form runs the chosen strengths through the host-window path). */
int size_search(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const PlTargetLayout &lay, const pngloss_hip_size_target &t,
                long bleed, hipStream_t stream, bool commit, pngloss_hip_result *results, pngloss_hip_zstream *streams, pngloss_hip_size_report *reports)
{
    SearchGuard guard{ ctx, false };
    const bool want_streams = commit && streams;
    SearchDevice dev{ ctx, images, lay, bleed, stream, {}, {} };
    std::vector<PlSizeTrack> st(n);
    auto has_pixels = [&](size_t i) { return images[i].width != 0 && images[i].height != 0; };
    for (size_t i = 0; i < n; i++) st[i].search = pl_size_begin(t.max_strength, has_pixels(i));
    /* one ordinary batch WITH emit descriptors: the images `who` at `strength`, their scanlines into the arena's probe regions */
    auto run_group = [&](uint32_t strength, const std::vector<uint32_t> &who) -> int {
        std::vector<EmitTarget> emits(who.size());
        std::vector<pngloss_hip_result> res;
        for (size_t k = 0; k < who.size(); k++) {
            const uint32_t pitch = lay.image[who[k]].pitch;
            emits[k] = EmitTarget{ pitch ? dev.address(who[k], PLA_IDS) : nullptr, pitch ? dev.address(who[k], PLA_ROWS) : nullptr, pitch };
        }
        int rc = dev.run(strength, who, emits.data(), res);
        if (rc) return rc;
        /* the group's out-flags words (colour type of the scanlines): gathered on the device, ONE copy */
        std::vector<PlMoveJob> gather;
        uint32_t *const d_flags = reinterpret_cast<uint32_t *>(dev.at(lay.flags));
        for (size_t k = 0; k < who.size(); k++) gather.push_back(PlMoveJob{ ctx->h_jobs[k].out_flags, d_flags + k, sizeof(uint32_t) });
        std::vector<uint32_t> flags(who.size(), 0);
        rc = dev.move(std::move(gather));
        if (rc) return rc;
        PL_CHECK(hipMemcpyAsync(flags.data(), d_flags, sizeof(uint32_t) * who.size(), hipMemcpyDeviceToHost, stream));
        PL_CHECK(hipStreamSynchronize(stream));
        for (size_t k = 0; k < who.size(); k++) {
            pl_search_ran(st[who[k]], strength, res[k]);
            st[who[k]].last.flags = (res[k].status == 0 && emits[k].pitch) ? flags[k] : 0;
        }
        return PNGLOSS_SUCCESS;
    };
    /* what the deflate is to look at: image i's scanlines in the probe region or in the stash, in the colour type `flags` says; out: where its stream goes, or nullptr */
    auto deflate_image = [&](size_t i, bool stash, uint32_t flags, const pngloss_hip_zstream *out) {
        return deflate_image_of(dev.address((uint32_t)i, stash ? PLA_BEST_IDS : PLA_IDS), dev.address((uint32_t)i, stash ? PLA_BEST_ROWS : PLA_ROWS), lay.image[i].pitch,
                                images[i].width * pl_emit_bpp_of(flags), images[i].height, out ? out->data : nullptr, out ? out->capacity : 0);
    };

    int rc = dev.move(pl_search_open(n));
    if (rc) return rc;
    for (;;) {
        const PlSearchRound round = pl_search_round(st);
        if (round.groups.empty()) break;
        rc = dev.move(round.back);
        for (size_t g = 0; g < round.groups.size() && rc == PNGLOSS_SUCCESS; g++) rc = run_group(round.groups[g].first, round.groups[g].second);      /* one after the other: a context takes one batch at a time */
        if (rc) return rc;
        /* ONE measuring deflate over every image probed in this round whose run succeeded */
        std::vector<pl_deflate_image> dz;
        std::vector<uint32_t> measured;
        for (uint32_t i : round.probed)
            if (st[i].last.result.status == 0) { dz.push_back(deflate_image(i, false, st[i].last.flags, nullptr)); measured.push_back(i); }
        std::vector<PlSizeRecord> sizes(dz.size());
        if (!dz.empty()) {
            rc = deflate_rc(pl_deflate_measure(dz.data(), dz.size(), sizes.data(), stream));
            if (rc) return rc;
        }
        for (size_t k = 0; k < measured.size(); k++) st[measured[k]].last.size = sizes[k];
        rc = dev.move(pl_size_settle(st, round.probed, t.max_bytes, want_streams));
        if (rc) return rc;
    }
    /* the kept results back into the images whose last probe was refused */
    rc = dev.move(pl_size_close(st, commit));
    if (rc) return rc;
    /* one launch of pl_distort: the kept results against the search's own originals, for the reports */
    std::vector<pngloss_hip_distortion> recs(n);
    if (commit && n) {
        std::vector<uint32_t> all(n);
        for (size_t i = 0; i < n; i++) all[i] = (uint32_t)i;
        rc = dev.distort(all, false, recs.data());
        if (rc) return rc;
    }
    PL_CHECK(hipStreamSynchronize(stream));
    /* one writing deflate over the kept results' scanlines: each stream's size is the measured size of the kept probe */
    if (want_streams) {
        std::vector<pl_deflate_image> dz;
        std::vector<size_t> who;
        for (size_t i = 0; i < n; i++) {
            zstream_clear(streams[i]);
            if (!has_pixels(i) || st[i].kept.result.status != 0) continue;
            streams[i].color_type = pl_color_type_of(st[i].kept.flags);
            dz.push_back(deflate_image(i, st[i].kept_in_stash, st[i].kept.flags, &streams[i]));
            who.push_back(i);
        }
        if (!dz.empty()) {
            rc = deflate_rc(pl_deflate_images(dz.data(), dz.size(), stream));
            if (rc) return rc;
        }
        for (size_t k = 0; k < dz.size(); k++) {
            pngloss_hip_zstream &z = streams[who[k]];
            zstream_take(z, dz[k]);
            if ((uint64_t)z.size != st[who[k]].kept.size.bytes) {
                std::fprintf(stderr, "pngloss_hip: image %zu: the written stream has %zu bytes, the measured one had %llu\n", who[k], z.size, (unsigned long long)st[who[k]].kept.size.bytes);
                return PNGLOSS_HIP_ERROR;
            }
        }
    }
    int worst = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < n; i++) {
        const PlSizeTrack &s = st[i];
        if (results) results[i] = s.kept.result;
        if (reports) {
            pngloss_hip_size_report r{};
            r.strength = s.search.chosen; r.probes = s.search.probes; r.runs = s.runs; r.reached = s.search.reached;
            r.bytes = s.kept.size.bytes;
            r.color_type = pl_color_type_of(s.kept.flags);
            r.distortion = recs[i];
            reports[i] = r;
        }
        if (s.kept.result.status) worst = PNGLOSS_INTERNAL_ABORT;
    }
    return worst;
}

/* One context's share of a search on host images, the one shape of both host forms.  Copies of the images go up into the search arena (laid out with the
 * SSIM tables and the scanline regions its caller names) and search(copies, layout, reports) -> code runs on them without committing; the host images stay as
 * they are until the chosen strengths run through the host-window path, once per distinct strength (pl_strength_groups) -- measured, so that every report
 * carries the record of what was written (with want_ssim the SSIM record too, into `ssim` where the caller has one; visible: both over visible pixels).  Report: .strength, .runs, .distortion.
 * empty_images_run: the rerun counts in the report of an image without pixels as well. */
template <class Report, class Search>
int batch_host_searched(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, long bleed_divider, pngloss_hip_result *results,
                        pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, Report *reports, bool want_ssim, bool visible, pngloss_hip_ssim *ssim,
                        int scanlines, bool empty_images_run, Search search)
{
    if (!ctx || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width, height, chosen(n);
    batch_dims(images, n, width, height);
    for (size_t i = 0; i < n; i++)
        if (width[i] && height[i] && !images[i].rgba) return PNGLOSS_INVALID_ARGUMENT;
    const PlTargetLayout lay = pl_target_layout(width, height, true, sizeof(PlMoveJob), sizeof(PlDistortJob), sizeof(PlDistortRecord),
                                                want_ssim ? sizeof(PlSsimJob) : 0, want_ssim ? sizeof(PlSsimRecord) : 0, scanlines);
    int rc = ctx->d_target.grow(lay.total, 8);
    if (rc == PNGLOSS_SUCCESS) rc = ensure_copy_stream(ctx);
    if (rc) return rc;
    std::vector<pngloss_hip_image_desc> descs(n);
    for (size_t i = 0; i < n; i++) {
        const size_t px = (size_t)width[i] * height[i];
        descs[i] = pngloss_hip_image_desc{ px ? ctx->d_target.p + lay.image[i].img : nullptr, (px && images[i].row_filters) ? ctx->d_target.p + lay.image[i].filters : nullptr, width[i], height[i] };
        if (px) PL_CHECK(hipMemcpyAsync(descs[i].d_rgba, images[i].rgba, px * 4, hipMemcpyHostToDevice, ctx->copy_stream));
    }
    PL_CHECK(hipStreamSynchronize(ctx->copy_stream));
    std::vector<Report> rep(n ? n : 1);
    SearchGuard guard{ ctx, true };       /* no single batch to index behind this call, here or on the peers */
    rc = search(descs.data(), lay, rep.data());
    if (pl_rc_is_hard(rc)) return rc;
    for (size_t i = 0; i < n; i++) chosen[i] = rep[i].strength;
    int worst = PNGLOSS_SUCCESS;
    for (const auto &group : pl_strength_groups(chosen)) {
        HostSubset sub(group.second, images, lines, zs);
        rc = batch_host(ctx, sub.images.data(), sub.n(), group.first, bleed_divider, Measure{ true, want_ssim, visible }, sub.results.data(), sub.lines(), sub.zs());
        sub.scatter(results, lines, zs);
        for (size_t k = 0; k < sub.n(); k++) {
            const size_t i = group.second[k];
            if (empty_images_run || (size_t)width[i] * height[i]) rep[i].runs++;
            if (pl_rc_is_hard(rc)) continue;
            (void)pngloss_hip_last_distortion(ctx, k, &rep[i].distortion);
            if (ssim && want_ssim) (void)pngloss_hip_last_ssim(ctx, k, &ssim[i]);
        }
        worst = pl_fold_rc(worst, rc);
    }
    if (reports) for (size_t i = 0; i < n; i++) reports[i] = rep[i];
    return worst;
}

/* one context's share of pngloss_hip_multi_optimize_batch_host_target: the rerun of the chosen strength counts for every image */
int batch_host_target(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_target2 &target, long bleed_divider,
                      pngloss_hip_result *results, pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, pngloss_hip_target_report *reports,
                      pngloss_hip_ssim *ssim)
{
    const bool visible = measure_of_options(ctx).visible;      /* option "measure": for the probes and for the records of the reruns */
    return batch_host_searched(ctx, images, n, bleed_divider, results, lines, zs, reports, target.min_ssim != 0.0, visible, ssim, PLT_SCANLINES_OFF, true,
                               [&](const pngloss_hip_image_desc *copies, const PlTargetLayout &lay, pngloss_hip_target_report *rep) {
                                   return target_search(ctx, copies, n, lay, target, visible, bleed_divider, ctx->copy_stream, false, nullptr, rep, nullptr);
                               });
}

/* one context's share of pngloss_hip_multi_optimize_batch_host_size: no SSIM, scanline regions for the probes, and the rerun of the chosen strength counts
 * only for an image that has pixels (one without ends with 0 runs) */
int batch_host_size(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_size_target &target, long bleed_divider,
                    pngloss_hip_result *results, pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, pngloss_hip_size_report *reports)
{
    /* the byte budget reports over all pixels, whatever the option "measure" says */
    return batch_host_searched(ctx, images, n, bleed_divider, results, lines, zs, reports, false, false, nullptr, PLT_SCANLINES_PROBE, false,
                               [&](const pngloss_hip_image_desc *copies, const PlTargetLayout &lay, pngloss_hip_size_report *rep) {
                                   return size_search(ctx, copies, n, lay, target, bleed_divider, ctx->copy_stream, false, nullptr, nullptr, rep);
                               });
}

/* ---- the argument checks of the entry points ---- */
int bleed_arguments(long bleed_divider)
{
    if (bleed_divider >= 1 && bleed_divider <= 32767) return PNGLOSS_SUCCESS;
    std::fprintf(stderr, "pngloss_hip: bleed must be 1..32767 (got %ld)\n", bleed_divider);
    return PNGLOSS_INVALID_ARGUMENT;
}

int target_arguments(const pngloss_hip_target2 *target, long bleed_divider)
{
    const int rc = pl_target_check2(target);
    if (rc) {
        std::fprintf(stderr, "pngloss_hip: the target needs min_psnr_db >= 0 (not NaN), max_abs_error 0..255, max_strength 0..255 and min_ssim 0..1 (not NaN)\n");
        return rc;
    }
    return bleed_arguments(bleed_divider);
}

int size_arguments(const pngloss_hip_size_target *target, const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, long bleed_divider)
{
    const int rc = pl_size_check(target, width.size(), width.data(), height.data());
    if (rc) {
        std::fprintf(stderr, "pngloss_hip: the size target needs max_strength 0..255, a budget above 0 for every image that has pixels, and images of at most 1 GiB of scanlines\n");
        return rc;
    }
    return bleed_arguments(bleed_divider);
}
} // namespace

extern "C" {

int pngloss_hip_optimize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                      const pngloss_hip_target *target, long bleed_divider, void *stream,
                                      pngloss_hip_result *results, pngloss_hip_target_report *reports)
{
    if (!target) return target_arguments(nullptr, bleed_divider);
    const pngloss_hip_target2 t2 = pl_target2_of(*target);
    return pngloss_hip_optimize_batch_target2(ctx, images, n, &t2, bleed_divider, stream, results, reports, nullptr);
}

int pngloss_hip_optimize_batch_target2(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                       const pngloss_hip_target2 *target, long bleed_divider, void *stream,
                                       pngloss_hip_result *results, pngloss_hip_target_report *reports, pngloss_hip_ssim *ssim)
{
    int rc = target_arguments(target, bleed_divider);
    if (rc) return rc;
    if (!ctx || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    if (previous_batch_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    for (size_t i = 0; i < n; i++)
        if (!images[i].d_rgba && width[i] && height[i]) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    /* room for every original and every best result beside the workspace -- or the call fails here, with no image touched */
    const bool want_ssim = target->min_ssim != 0.0;
    const PlTargetLayout lay = pl_target_layout(width, height, false, sizeof(PlMoveJob), sizeof(PlDistortJob), sizeof(PlDistortRecord),
                                                want_ssim ? sizeof(PlSsimJob) : 0, want_ssim ? sizeof(PlSsimRecord) : 0);
    rc = ctx->d_target.grow(lay.total, 8);
    if (rc) return rc;
    return target_search(ctx, images, n, lay, *target, ctx->opt_visible, bleed_divider, static_cast<hipStream_t>(stream), true, results, reports, ssim);
}

int pngloss_hip_multi_optimize_batch_host_target(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                                 const pngloss_hip_target *target, long bleed_divider, pngloss_hip_result *results,
                                                 pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                                 pngloss_hip_target_report *reports)
{
    if (!target) return target_arguments(nullptr, bleed_divider);
    const pngloss_hip_target2 t2 = pl_target2_of(*target);
    return pngloss_hip_multi_optimize_batch_host_target2(m, images, n, &t2, bleed_divider, results, scanlines, streams, reports, nullptr);
}

int pngloss_hip_multi_optimize_batch_host_target2(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                                  const pngloss_hip_target2 *target, long bleed_divider, pngloss_hip_result *results,
                                                  pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                                  pngloss_hip_target_report *reports, pngloss_hip_ssim *ssim)
{
    const int arc = target_arguments(target, bleed_divider);
    if (arc) return arc;
    if (!m || m->ctx.empty() || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    return deal_over_contexts(m, images, n, results, scanlines, streams, false, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        std::vector<pngloss_hip_target_report> rp(mine.n());
        std::vector<pngloss_hip_ssim> sm(mine.n());
        const int rc = batch_host_target(ctx, mine.images.data(), mine.n(), *target, bleed_divider, mine.results.data(), mine.lines(), mine.zs(), rp.data(), sm.data());
        for (size_t k = 0; k < mine.n(); k++) {
            if (reports) reports[mine.who[k]] = rp[k];
            if (ssim && target->min_ssim != 0.0) ssim[mine.who[k]] = sm[k];
        }
        return rc;
    });
}

int pngloss_hip_optimize_batch_size(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                    const pngloss_hip_size_target *target, long bleed_divider, void *stream,
                                    pngloss_hip_result *results, pngloss_hip_zstream *streams, pngloss_hip_size_report *reports)
{
    if (n && !images) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<uint32_t> width, height;
    batch_dims(images, n, width, height);
    int rc = size_arguments(target, width, height, bleed_divider);
    if (rc) return rc;
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    if (previous_batch_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; i++) {
        if (!images[i].d_rgba && width[i] && height[i]) return PNGLOSS_INVALID_ARGUMENT;
        if (streams && width[i] && height[i] && (!streams[i].data || streams[i].capacity < pl_deflate_bound(width[i], height[i]))) return PNGLOSS_INVALID_ARGUMENT;
    }
    PL_CHECK(hipSetDevice(ctx->device));
    /* room for every original, every best result and the scanlines beside the workspace -- or the call fails here, with no image touched */
    const PlTargetLayout lay = pl_target_layout(width, height, false, sizeof(PlMoveJob), sizeof(PlDistortJob), sizeof(PlDistortRecord), 0, 0,
                                                streams ? PLT_SCANLINES_PROBE_AND_BEST : PLT_SCANLINES_PROBE);
    rc = ctx->d_target.grow(lay.total, 8);
    if (rc) return rc;
    return size_search(ctx, images, n, lay, *target, bleed_divider, static_cast<hipStream_t>(stream), true, results, streams, reports);
}

int pngloss_hip_multi_optimize_batch_host_size(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                               const pngloss_hip_size_target *target, long bleed_divider, pngloss_hip_result *results,
                                               pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                               pngloss_hip_size_report *reports)
{
    if (n && !images) return PNGLOSS_INVALID_ARGUMENT;
    {
        std::vector<uint32_t> width, height;
        batch_dims(images, n, width, height);
        const int arc = size_arguments(target, width, height, bleed_divider);
        if (arc) return arc;
    }
    if (!m || m->ctx.empty()) return PNGLOSS_INVALID_ARGUMENT;
    return deal_over_contexts(m, images, n, results, scanlines, streams, false, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        std::vector<pngloss_hip_size_report> rp(mine.n());
        std::vector<uint64_t> budget(mine.n(), 0);
        for (size_t k = 0; k < mine.n(); k++) if (target->max_bytes) budget[k] = target->max_bytes[mine.who[k]];
        const pngloss_hip_size_target mine_t = { budget.data(), target->max_strength, 0 };
        const int rc = batch_host_size(ctx, mine.images.data(), mine.n(), mine_t, bleed_divider, mine.results.data(), mine.lines(), mine.zs(), rp.data());
        for (size_t k = 0; k < mine.n(); k++) if (reports) reports[mine.who[k]] = rp[k];
        return rc;
    });
}

} /* extern "C" */

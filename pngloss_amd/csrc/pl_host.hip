/*
 * pl_host.hip -- the core of the thin C-ABI shim of libpngloss_hip.so (see include/pngloss_hip.h for the contract): the context's life, the caller's
 * options, the batch pipeline (enqueue, finish, the engine report), the plain optimize_batch* entry points, pngloss_hip_last_*, and the host-pointer
 * drop-in entry points that replace the reference's src/pngloss_image.c:29-156.  pl_host_ctx.h has the map of the other host files and says which
 * file may write which member of the context.
 *
 * Host side only: no arithmetic of the hot path is done here and there is no CPU fallback: without a usable HIP device every entry point fails
 * loudly.  What ONE call asks of a batch -- strength, stream, emit targets, a synchronous caller, what to measure behind it -- is an argument
 * (BatchCall) of enqueue: no function tells another what to run by writing into the context.
 */
#include "pl_host_ctx.h"

/* the hooks of the environment (PlHooks, pl_plan.h): read once, when a context is created */
static PlHooks from_env()
{
    PlHooks h;
    auto num = [](const char *name, int dflt) { const char *e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    if (std::getenv("PNGLOSS_HIP_SEG_GROUPS")) h.seg_groups = std::max(1, std::min(SEG_MAX_GROUPS, num("PNGLOSS_HIP_SEG_GROUPS", 0)));
    h.no_stream_wait = std::getenv("PNGLOSS_HIP_NO_STREAM_WAIT") != nullptr;
    if (std::getenv("PNGLOSS_HIP_SEG_UNIT")) h.seg_unit = num("PNGLOSS_HIP_SEG_UNIT", 0) != 0 ? 1 : 0;
    h.tparts = num("PNGLOSS_HIP_SEG_TPARTS", 0);
    h.enum_nt = num("PNGLOSS_HIP_ENUM_NT", 0);
    h.kin = num("PNGLOSS_HIP_KIN", -1);
    h.seg_seeds = num("PNGLOSS_HIP_SEG_SEEDS", -1);
    h.seg_seeds1 = num("PNGLOSS_HIP_SEG_SEEDS1", -1);
    h.pin = num("PNGLOSS_HIP_PIN", -1);
    h.calib = num("PNGLOSS_HIP_CALIB", -1);
    h.seed_kin = num("PNGLOSS_HIP_SEED_KIN", -1);
    h.segprof = std::getenv("PNGLOSS_HIP_SEGPROF") != nullptr;
    h.debug = std::getenv("PNGLOSS_HIP_DEBUG") != nullptr;
    h.debug_seam = std::getenv("PNGLOSS_HIP_DEBUG_SEAM") != nullptr;
    h.force_careful = std::getenv("PNGLOSS_HIP_FORCE_CAREFUL") != nullptr;
    { const char *no = std::getenv("PNGLOSS_HIP_NO_SPLIT"); h.no_split = no && *no == '1'; }
    { const int v = num("PNGLOSS_HIP_SPLIT", 0); if (v >= 1 && v <= 8) h.split = v; }
    return h;
}

void forget_last_batch(pngloss_hip_ctx *c)
{
    c->n_last = 0; c->h_jobs.clear(); c->distortion.clear(); c->d_records = nullptr; c->ssim.clear(); c->d_ssim_records = nullptr; c->palette.clear(); c->index_depth.clear(); c->split_last = false;
}

namespace {

float recip_up_host(long d)
{
    /* one ulp above the correctly rounded reciprocal: > 1/d, and far inside the exactness margin (pl_device.h) */
    float r = 1.0f / (float)d;
    r = std::nextafterf(r, 2.0f);
    return r;
}

/* ---- the cost model that picks a batch's row engine: an OPTIONAL calibration per device (PNGLOSS_HIP_CALIB=1) ------------------------------
 * Its constants were fitted on one kind of box (MI355X, 256 CUs, performance level "auto").  Round 6 (the review's item): with the switch, the first batch of two or more images
 * whose engine is the library's to choose runs a small synthetic image (1024 x 32, photographic) three times on each engine through a context of its own -- ~30 ms, once per
 * device and process -- and compares with what the reference box takes for it; the model's per-attempt floor and per-pixel cost are scaled by the ratios (dead band 15 %).
 * OFF by default (enqueue says why: a probe that short reads the clock governor).  What is always taken from the device is its CU count: the model's per-workgroup slope and its
 * "one image per CU" terms.  pngloss_hip_last_engine_info does not change: it reports what ran. */
struct EngineCalib { double seg = 1.0, wg = 1.0, cus = 256.0; double seg_ms = 0, wg_ms = 0; bool done = false; };
constexpr double CALIB_REF_SEG_MS = 2.40, CALIB_REF_WG_MS = 5.97;      /* (the reference box, profiles/r06_host_side.txt: min of three runs of the 1024 x 32 image, five processes: 2.39 .. 2.42 and 5.94 .. 6.04 ms) */
std::mutex g_calib_mu;
EngineCalib g_calib[32];
thread_local bool t_calibrating = false;
EngineCalib engine_calib(int device, bool debug)
{
    std::lock_guard<std::mutex> lk(g_calib_mu);
    EngineCalib &c = g_calib[device & 31];
    if (c.done || t_calibrating) return c;
    c.done = true;                                       /* (whatever happens below: once) */
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c.cus = (double)cus;
    t_calibrating = true;
    pngloss_hip_ctx *tmp = pngloss_hip_create(device);
    const uint32_t w = 1024, h = 32;
    std::vector<uint32_t> img((size_t)w * h);
    uint32_t lcg = 12345u;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            lcg = lcg * 1664525u + 1013904223u;
            const uint32_t r = std::min(255u, x * 255u / w + ((lcg >> 8) & 7u)), g = std::min(255u, y * 255u / h + ((lcg >> 12) & 7u)), b = std::min(255u, (x + y) * 255u / (w + h) + ((lcg >> 16) & 7u));
            img[(size_t)y * w + x] = r | (g << 8) | (b << 16) | ((255u - ((x ^ y) & 31u)) << 24);
        }
    void *d_img = nullptr, *d_f = nullptr;
    bool ok = tmp && hipMalloc(&d_img, img.size() * 4) == hipSuccess && hipMalloc(&d_f, h) == hipSuccess;
    double ms[2] = { 0, 0 };
    for (int e = 0; e < 2 && ok; e++) {
        tmp->opt_engine = e == 0 ? PlEnginePin::Seg : PlEnginePin::Wg;
        double best = 1e30;
        for (int rep = 0; rep < 3 && ok; rep++) {
            ok = hipMemcpy(d_img, img.data(), img.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
            pngloss_hip_image_desc desc{ d_img, d_f, w, h };
            pngloss_hip_result res{};
            if (ok) ok = pngloss_hip_optimize_batch(tmp, &desc, 1, 19, 2, nullptr, &res) == PNGLOSS_SUCCESS && res.status == 0;
            if (ok) best = std::min(best, pngloss_hip_last_engine_ms(tmp));
        }
        ms[e] = best;
    }
    if (d_img) (void)hipFree(d_img);
    if (d_f) (void)hipFree(d_f);
    if (tmp) pngloss_hip_destroy(tmp);
    t_calibrating = false;
    if (ok && ms[0] > 0 && ms[1] > 0) {
        c.seg_ms = ms[0]; c.wg_ms = ms[1];
        const double rs = ms[0] / CALIB_REF_SEG_MS, rw = ms[1] / CALIB_REF_WG_MS, ratio = rs / rw;
        if (ratio < 0.85 || ratio > 1.0 / 0.85) { c.seg = std::min(2.0, std::max(0.5, rs)); c.wg = std::min(2.0, std::max(0.5, rw)); }
    }
    if (debug) std::fprintf(stderr, "pngloss_hip: engine calibration on device %d: %g CUs, 1024x32 frame: segment engine %.3f ms (reference %.2f), workgroup engine %.3f ms (reference %.2f) -> cost model scales %.2f / %.2f\n",
                            device, c.cus, ms[0], CALIB_REF_SEG_MS, ms[1], CALIB_REF_WG_MS, c.seg, c.wg);
    return c;
}

} // namespace

int enqueue(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const BatchCall &call)
{
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    const unsigned strength = call.strength; const long bleed = call.bleed;
    const hipStream_t stream = call.stream;
    if (strength > 255 || bleed < 1 || bleed > 32767) {
        std::fprintf(stderr, "pngloss_hip: strength must be 0..255 and bleed 1..32767 (got %u, %ld)\n", strength, bleed);
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (previous_batch_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    if (ctx->seg_worker.joinable()) ctx->seg_worker.join();          /* (a batch that failed half-way) */
    forget_last_batch(ctx);
    const bool distort = call.measure.distortion, ssim = call.measure.ssim, visible = call.measure.visible;
    const bool keep_originals = distort || ssim;     /* one arena, one pl_keep launch, whichever of the two options wants the originals */
    const PlHooks &hk = ctx->hooks;
    PlPlanInput in;
    in.strength = strength; in.bleed = bleed; in.hooks = hk;
    /* the pin of the row engine: the option of the ABI first; the environment variable is the tests' hook (the one hook read per call, once: here) */
    const char *const env_engine = ctx->opt_engine == PlEnginePin::Auto ? std::getenv("PNGLOSS_HIP_ENGINE") : nullptr;
    in.pin = ctx->opt_engine != PlEnginePin::Auto ? ctx->opt_engine : pl_engine_pin_of_env(env_engine);
    const bool engine_named = ctx->opt_engine != PlEnginePin::Auto || (env_engine && *env_engine);
#ifdef PL_DEBUG_FORCE_FILTER
    in.forced_filter = PL_DEBUG_FORCE_FILTER;   /* (a debugging BUILD: candidate PL_DEBUG_FORCE_FILTER wins every row -- not the reference's bytes; pngloss_hip_version says so) */
#endif
    if (pl_rows_wanted(strength, in.pin, hk, in.forced_filter)) {
        /* the row-statistics engine keeps PL_ROWSTAT_WORDS counters per ROW of every image (5.6 MB per 1080p frame: 2.8 GB for 512 frames) -- the other engines need nothing
         * comparable.  A batch whose counters would not fit beside its images runs strength 0 the long way (the segment / workgroup engines) instead of failing: same bytes. */
        size_t rs = 0, free_b = 0, total_b = 0;
        for (size_t i = 0; i < n; i++) rs += pl_rowstat_bytes(images[i].height);
        const size_t have = ctx->d_ws.bytes;                      /* (what the context's arena already holds counts as available) */
        if (rs > have && hipMemGetInfo(&free_b, &total_b) == hipSuccess && rs - have > free_b / 2) {
            if (hk.debug) std::fprintf(stderr, "pngloss_hip: strength 0: %zu MB of row counters against %zu MB free: using the other row engines for this batch\n", rs >> 20, free_b >> 20);
            in.rows_fit = false;
        }
    }
    for (size_t i = 0; i < n; i++)
        if (!images[i].d_rgba && images[i].width && images[i].height) return PNGLOSS_INVALID_ARGUMENT;
    batch_dims(images, n, in.width, in.height);
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0) in.cus = (double)cus; }
    in.sync_call = call.sync_call; in.three_groups_ok = call.three_groups_ok; in.opt_launch_groups = ctx->opt_launch_groups;
    in.stream_wait_used = g_stream_wait_used.load(std::memory_order_relaxed);
    PlPlan plan = pl_plan_batch(in);
    /* OPT-IN (PNGLOSS_HIP_CALIB=1) since it was measured inside bench.py: the probe is 2 - 6 ms of GPU work, and what it finds depends on what the process did before it
     * (the clock governor follows the load: after the headline's steps the probe read the segment engine 1.3x slower against the other one than in a fresh process, the
     * model sent 128 frames of 1080p to the wrong engine and the 256-frame batch lost 16 %: profiles/r06_host_side.txt).  A wrong calibration costs more than the constants
     * of the reference box cost on a box of another kind; the CU count (deterministic) is always taken from the device. */
    if (plan.seg_costed && !engine_named && n >= 2 && hk.calib > 0 && !t_calibrating) {
        const EngineCalib cal = engine_calib(ctx->device, hk.debug);
        in.cus = cal.cus; in.seg_scale = cal.seg; in.wg_scale = cal.wg;
        plan = pl_plan_batch(in);
    }
    if (plan.seg_pin_unmet)
        std::fprintf(stderr, "pngloss_hip: PNGLOSS_HIP_ENGINE=seg: nothing in this batch for the segment engine (widths beyond %u?); using the one-workgroup-per-image engine\n", SEG_MAX_WIDTH);
    const bool use_rows = plan.use_rows, use_seg = !plan.seg_list.empty();
    const std::vector<uint32_t> &wg_list = plan.wg_list;
    const PlBatchLayout lay = pl_batch_layout(in.width, in.height, use_rows, plan.seg_list, wg_list.size(), (uint32_t)plan.params.nsp, plan.params.seeded != 0,
                                              sizeof(PlJob), sizeof(SegJob));
    int rc = ctx->d_ws.grow(lay.total, 4);
    if (rc) return rc;
    /* options "distortion" and "ssim": room for every original beside the workspace -- or the call fails here, with nothing enqueued */
    PlKeepLayout keep;
    if (keep_originals) {
        keep = pl_keep_layout(in.width, in.height, true, sizeof(PlDistortJob), sizeof(PlDistortRecord));
        rc = ctx->d_keep.grow(keep.total, 8);
        if (rc) return rc;
    }
    for (size_t i = 0; i < n; i++) {
        const WsLayout &l = lay.ws[i];
        char *b = ctx->d_ws.p + lay.image[i];
        PlJob j{};
        j.rowstat = use_rows ? reinterpret_cast<uint32_t *>(b + l.rowstat) : nullptr;
        j.img = static_cast<uint32_t *>(images[i].d_rgba);
        j.row_filters = static_cast<uint8_t *>(images[i].d_row_filters);
        j.width = images[i].width;
        j.height = (images[i].width == 0) ? 0 : images[i].height;
        j.forced_bpp = call.forced_bpp ? call.forced_bpp[i] : 0;
        j.flags = reinterpret_cast<uint32_t *>(b + l.flags);
        j.orig_hist = reinterpret_cast<uint32_t *>(b + l.orig_hist);
        j.orig_rank = reinterpret_cast<uint32_t *>(b + l.orig_rank);
        j.cand = reinterpret_cast<uint4 *>(b + l.cand);
        j.err0 = reinterpret_cast<uint2 *>(b + l.err0);
        j.err1 = reinterpret_cast<uint2 *>(b + l.err1);
        j.old_above = reinterpret_cast<uint32_t *>(b + l.old_above);
        j.final_hist = reinterpret_cast<uint32_t *>(b + l.final_hist);
        j.result = reinterpret_cast<int32_t *>(b + l.result);
        j.row_ids = reinterpret_cast<uint8_t *>(b + l.row_ids);
        j.out_flags = reinterpret_cast<uint32_t *>(b + l.out_flags);
        if (call.emits && call.emits[i].d_rows) {
            j.emit_ids = static_cast<uint8_t *>(call.emits[i].d_ids);
            j.emit_rows = static_cast<uint8_t *>(call.emits[i].d_rows);
            j.emit_pitch = call.emits[i].pitch;
            j.emit_adaptive_all = images[i].d_row_filters ? 0u : 1u;
        }
        j.progress = nullptr;
        if (call.want_progress && i == 0 && ctx->h_progress) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, ctx->h_progress, 0) == hipSuccess) j.progress = static_cast<uint32_t *>(dp);
        }
        ctx->h_jobs.push_back(j);
    }
    if (!n) return PNGLOSS_SUCCESS;
    PlJob *d_jobs = reinterpret_cast<PlJob *>(ctx->d_ws.p);
    PL_CHECK(hipMemcpyAsync(d_jobs, ctx->h_jobs.data(), sizeof(PlJob) * n, hipMemcpyHostToDevice, stream));

    PlEngineParams prm{};
    prm.strength = (int)strength;
    prm.rq = recip_up_host((long)strength + 1);
    prm.rbleed = recip_up_host(bleed);
    prm.r29 = 2.0f * recip_up_host(9);
    prm.force_careful = hk.force_careful;   /* test hook, see pl_device.h */
    prm.engine_mode = plan.engine_mode;

    const PlDistortJob *const d_dj = keep_originals ? reinterpret_cast<const PlDistortJob *>(ctx->d_keep.p + keep.jobs) : nullptr;
    uint64_t max_pixels = 0, max_tiles = 0;
    PlSsimLayout ssim_lay;
    if (keep_originals) {
        std::vector<const void *> img(n);
        std::vector<uint64_t> pixels(n);
        for (size_t i = 0; i < n; i++) {
            img[i] = images[i].d_rgba;
            pixels[i] = (uint64_t)images[i].width * images[i].height;
            max_pixels = std::max(max_pixels, pixels[i]);
        }
        rc = upload_distort_jobs(ctx, keep, n, img.data(), nullptr, pixels.data(), stream);
        if (rc) return rc;
        if (ssim) {
            std::vector<const void *> orig(n);
            for (size_t i = 0; i < n; i++) orig[i] = ctx->d_keep.p + keep.image[i];
            rc = upload_ssim_jobs(ctx, n, orig.data(), img.data(), in.width.data(), in.height.data(), stream, ssim_lay, max_tiles, visible);
            if (rc) return rc;
        }
    }
    PL_CHECK(hipEventRecord(ctx->ev[0], stream));
    if (keep_originals) PL_CHECK(pl_launch_keep(d_dj, n, max_pixels, stream));      /* the originals, before pl_classify / pl_repack rewrite the images in place */
    PL_CHECK(pl_launch_prepare(d_jobs, ctx->h_jobs.data(), n, stream, !use_rows));
    ctx->engine.assign(n, (uint8_t)(use_rows ? PLR_ENGINE_ROWS : PLR_ENGINE_WG));
    for (uint32_t i : plan.seg_list) ctx->engine[i] = (uint8_t)PLR_ENGINE_SEG;
    PL_CHECK(hipEventRecord(ctx->ev[1], stream));
    /* the images of the one-workgroup-per-image engine: all of them, or -- a mixed batch -- those the segment engine did not get; they
     * run on the caller's stream while the segment engine works on its own */
    const uint32_t *d_sel = nullptr;
    if (use_seg && !wg_list.empty()) {
        ctx->h_sel = wg_list;
        PL_CHECK(hipMemcpyAsync(ctx->d_ws.p + lay.sel, ctx->h_sel.data(), sizeof(uint32_t) * wg_list.size(), hipMemcpyHostToDevice, stream));
        d_sel = reinterpret_cast<const uint32_t *>(ctx->d_ws.p + lay.sel);
    }
    if (use_seg) {
        rc = run_seg_engine(ctx, d_jobs, plan, lay, call, d_sel, prm);
        if (rc) return rc;
    } else if (use_rows) PL_CHECK(pl_launch_rows(d_jobs, ctx->h_jobs.data(), n, stream));
    else PL_CHECK(pl_launch_engine(d_jobs, nullptr, n, prm, stream));
    PL_CHECK(hipEventRecord(ctx->ev[2], stream));
    {
        /* (behind this point the segment engine's launch thread may be running: it is joined before an error is returned) */
        hipError_t e = pl_launch_finish(d_jobs, ctx->h_jobs.data(), n, stream);
        if (e == hipSuccess && distort) e = pl_launch_distort(d_dj, n, max_pixels, stream, visible);      /* behind pl_unpack: the final RGBA8 against the kept original */
        if (e == hipSuccess && ssim) e = pl_launch_ssim(reinterpret_cast<const PlSsimJob *>(ctx->d_ssim.p + ssim_lay.jobs), n, max_tiles, stream, visible);
        if (e == hipSuccess) e = pl_launch_emit(d_jobs, ctx->h_jobs.data(), n, stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev[3], stream);
        if (e != hipSuccess) {
            std::fprintf(stderr, "pngloss_hip: enqueueing the kernels behind the row engine failed: %s\n", hipGetErrorString(e));
            if (ctx->seg_worker.joinable()) ctx->seg_worker.join();
            for (int g = 0; g < SEG_MAX_GROUPS; g++) if (ctx->seg_gstream[g]) (void)hipStreamSynchronize(ctx->seg_gstream[g]);
            return PNGLOSS_HIP_ERROR;
        }
    }
    ctx->n_last = n;
    if (distort) ctx->d_records = reinterpret_cast<const PlDistortRecord *>(ctx->d_keep.p + keep.records);
    if (ssim) ctx->d_ssim_records = reinterpret_cast<const PlSsimRecord *>(ctx->d_ssim.p + ssim_lay.records);
    ctx->pending = true;
    return PNGLOSS_SUCCESS;
}

/* PNGLOSS_HIP_DEBUG / PNGLOSS_HIP_SEGPROF: what the row engine did for image i of the batch just finished, from its record r (pl_result.h) and the
 * engine the plan gave it.  tools/ab_*.sh grep these lines ("engine [0-9.]* ms"). */
static void print_engine_report(const pngloss_hip_ctx *ctx, size_t i, const int32_t *r, int engine)
{
    const PlHooks &hk = ctx->hooks;
    if (i == 0 && hk.debug) std::fprintf(stderr, "pngloss_hip: row engine occupancy query: %d workgroups per CU\n", pl_engine_occupancy());
    if (engine == PLR_ENGINE_SEG) {
        if (hk.debug)
            std::fprintf(stderr, "pngloss_hip: image %zu: segment-parallel engine: %d attempts for %u rows, %d epochs (validation restarts), %d rows finished serially, candidate none dropped by its cost bound %d times, %d segments walked step by step by the chain kernel, engine %.3f ms\n",
                         i, r[PLR_SEG_ATTEMPTS], ctx->h_jobs[i].height, r[PLR_REPAIRED], r[PLR_SEG_SERIAL_ROWS], r[PLR_SEG_NONE_DROPPED], r[PLR_SEG_WALKED], ctx->engine_ms);
        if (!hk.segprof) return;
        /* the phase clocks (100 MHz ticks), in us: the slowest workgroup, and the average over the `runs` workgroups that added to a sum */
        auto mx = [&](int slot) { return r[slot] / 100.0; };
        auto avg = [&](int sum, int runs) { return (uint32_t)r[sum] / 100.0 / (uint32_t)r[runs]; };
        const int cand = PLR_SEG_CAND_RUNS, commit = PLR_SEG_COMMIT_RUNS, en = PLR_SEG_ENUM_RUNS, ch = PLR_SEG_CHAIN_RUNS, val = PLR_SEG_VAL_RUNS;
        std::fprintf(stderr, "pngloss_hip:   validation kernel, slowest workgroup per phase (us): load %.1f  pass1 %.1f  watched bins + pass3 %.1f  none bound %.1f  sums %.1f; pending decisions %d\n",
                     mx(PLR_SEG_VAL_MAX), mx(PLR_SEG_VAL_MAX + 1), mx(PLR_SEG_VAL_MAX + 2), mx(PLR_SEG_VAL_MAX + 3), mx(PLR_SEG_VAL_MAX + 4), r[PLR_SEG_VAL_PENDING]);
        std::fprintf(stderr, "pngloss_hip:   control kernel, slowest (us): candidate workgroup up to the table build %.1f, table build %.1f, commit workgroup %.1f\n",
                     mx(PLR_SEG_CTL_MAX), mx(PLR_SEG_CTL_MAX + 1), mx(PLR_SEG_CTL_MAX + 2));
        if (r[cand] && r[commit])
            std::fprintf(stderr, "pngloss_hip:   ... average (us): candidate workgroup up to the table build %.2f, table build %.2f, commit workgroup %.2f\n",
                         avg(PLR_SEG_CAND_SUM, cand), avg(PLR_SEG_CAND_SUM + 1, cand), avg(PLR_SEG_COMMIT_SUM, commit));
        if (r[cand])
            std::fprintf(stderr, "pngloss_hip:   ... candidate workgroup, average (us): requests + copy %.2f, decision %.2f, new histogram + fields %.2f\n",
                         avg(PLR_SEG_CAND_REQ_SUM, cand), avg(PLR_SEG_CAND_DECIDE_SUM, cand), avg(PLR_SEG_CAND_HIST_SUM, cand));
        if (r[cand])
            std::fprintf(stderr, "pngloss_hip:   ... commit workgroup, average (us): requests + copy %.2f, decision %.2f, terms %.2f, rows + extremes %.2f\n",
                         avg(PLR_SEG_COMMIT_REQ_SUM, commit), avg(PLR_SEG_COMMIT_DECIDE_SUM, commit), avg(PLR_SEG_COMMIT_TERMS_SUM, commit), avg(PLR_SEG_COMMIT_ROWS_SUM, commit));
        if (r[cand])
            std::fprintf(stderr, "pngloss_hip:   ... table build, average (us): keys %.2f, classes %.2f, entries + write %.2f\n",
                         avg(PLR_SEG_TABLE_SUM, cand), avg(PLR_SEG_TABLE_SUM + 1, cand), avg(PLR_SEG_TABLE_SUM + 2, cand));
        if (r[en])
            std::fprintf(stderr, "pngloss_hip:   enumeration workgroups (us), slowest / average: load %.1f / %.2f  first steps (%d, or %d for a state set of one chunk) + dedupe %.1f / %.2f  remaining steps %.1f / %.2f  map %.1f / %.2f; distinct states per channel after the dedupe %.1f; first-segment walker %.1f / %.2f\n",
                         mx(PLR_SEG_ENUM_MAX), avg(PLR_SEG_ENUM_SUM, en), SEG_K1, SEG_K1_ONE_CHUNK, mx(PLR_SEG_ENUM_MAX + 1), avg(PLR_SEG_ENUM_SUM + 1, en),
                         mx(PLR_SEG_ENUM_MAX + 2), avg(PLR_SEG_ENUM_SUM + 2, en), mx(PLR_SEG_ENUM_MAX + 3), avg(PLR_SEG_ENUM_SUM + 3, en),
                         (uint32_t)r[PLR_SEG_ENUM_STATES] / 4.0 / (uint32_t)r[en], mx(PLR_SEG_FIRST_MAX), r[PLR_SEG_FIRST_RUNS] ? avg(PLR_SEG_FIRST_SUM, PLR_SEG_FIRST_RUNS) : 0.0);
        if (r[ch])
            std::fprintf(stderr, "pngloss_hip:   chain workgroups (us), slowest / average: gather %.1f / %.2f  compose %.1f / %.2f  walk %.1f / %.2f  tail %.1f / %.2f; %u runs, %u through the serial walk, %u at the wide stride\n",
                         mx(PLR_SEG_CHAIN_MAX), avg(PLR_SEG_CHAIN_SUM, ch), mx(PLR_SEG_CHAIN_MAX + 1), avg(PLR_SEG_CHAIN_SUM + 1, ch), mx(PLR_SEG_CHAIN_MAX + 2), avg(PLR_SEG_CHAIN_SUM + 2, ch),
                         mx(PLR_SEG_CHAIN_MAX + 3), avg(PLR_SEG_CHAIN_SUM + 3, ch), (uint32_t)r[ch], (uint32_t)r[PLR_SEG_WALKED], (uint32_t)r[PLR_SEG_CHAIN_WIDE]);
        if (r[val])
            std::fprintf(stderr, "pngloss_hip:   ... average per workgroup (us): load %.2f  pass1 %.2f  watched bins + pass3 %.2f  none bound %.2f  sums %.2f  (%u workgroup runs)\n",
                         avg(PLR_SEG_VAL_SUM, val), avg(PLR_SEG_VAL_SUM + 1, val), avg(PLR_SEG_VAL_SUM + 2, val), avg(PLR_SEG_VAL_SUM + 3, val), avg(PLR_SEG_VAL_SUM + 4, val), (uint32_t)r[val]);
        return;
    }
    /* the workgroup engine's slots (the row-statistics engine leaves them 0) */
    if (!hk.debug) return;
    const int32_t *kc = r + PLR_WG_CHAIN_KCYC, *slow = r + PLR_WG_SLOW_PX, *light = r + PLR_WG_LIGHT_PX, *flush = r + PLR_WG_FLUSH_KCYC, *cpp = r + PLR_WG_CYC_PER_PX;
    const bool lead = r[PLR_WG_LEAD_ROWS] != 0;
    std::fprintf(stderr, "pngloss_hip: image %zu: chain kcycles per wave %d %d %d %d, repaired pixels %d %d %d %d, engine %.3f ms\n", i,
                 kc[0], kc[1], kc[2], kc[3], slow[0], slow[1], slow[2], slow[3], ctx->engine_ms);
    std::fprintf(stderr, "pngloss_hip: image %zu: band-leader row attempts %d, wave 4 kcycles %d, exact redos %d, band rescans (wave 0 / 4) %d %d\n", i,
                 r[PLR_WG_LEAD_ROWS], r[PLR_WG_W4_KCYC], r[PLR_WG_W4_SLOW_PX], r[PLR_WG_RESCANS], r[PLR_WG_W4_RESCANS]);
    if (lead)
        for (int w = 0; w < PLR_WG_WAVES; w++) {
            const int32_t *ph = r + PLR_WG_PHASE_KCYC + PLR_WG_PHASES * w;
            std::fprintf(stderr, "pngloss_hip:   wave %d (%s) kcycles: vector %d  fast groups %d  exact redo %d  rescan %d  table build %d\n", w,
                         w == 0 ? "up" : (w == 1 ? "sub" : (w == 2 ? "average" : (w == 3 ? "paeth" : "none"))), ph[0], ph[1], ph[2], ph[3], ph[4]);
        }
    if (lead)
        std::fprintf(stderr, "pngloss_hip:   cycles per pixel of undisturbed whole-chunk runs (up sub average paeth none): %d %d %d %d %d\n", cpp[0], cpp[1], cpp[2], cpp[3], cpp[4]);
    std::fprintf(stderr, "pngloss_hip:   wave 0 kcycles in the post pass %d, in the commit pass %d; flush + relation check per chain wave %d %d %d %d %d\n",
                 r[PLR_WG_POST_KCYC], r[PLR_WG_COMMIT_KCYC], flush[0], flush[1], flush[2], flush[3], flush[4]);
    const int32_t m = r[PLR_WG_SIMD_MAP];
    std::fprintf(stderr, "pngloss_hip:   SIMD of waves 0..7: %d %d %d %d %d %d %d %d\n", m & 3, (m >> 2) & 3, (m >> 4) & 3, (m >> 6) & 3,
                 (m >> 8) & 3, (m >> 10) & 3, (m >> 12) & 3, (m >> 14) & 3);
    if (lead)
        std::fprintf(stderr, "pngloss_hip:   light pixels per chain wave %d %d %d %d %d; rows on the round-1 chains by the adaptive choice %d (last cycles per pixel: band-leader %d, round-1 %d)\n",
                     light[0], light[1], light[2], light[3], light[4], r[PLR_WG_ADAPT_LEGACY], r[PLR_WG_EST_LEAD], r[PLR_WG_EST_LEGACY]);
}

int finish(pngloss_hip_ctx *ctx, pngloss_hip_result *results, size_t n)
{
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    if (!ctx->pending) {
        if (results)
            for (size_t i = 0; i < n; i++) results[i] = pngloss_hip_result{ 0, 0, 0, 0, 0 };
        return PNGLOSS_SUCCESS;
    }
    PL_CHECK(hipSetDevice(ctx->device));
    int seg_rc = PNGLOSS_SUCCESS;
    if (ctx->seg_worker.joinable()) {
        ctx->seg_worker.join();
        seg_rc = ctx->seg_rc.load(std::memory_order_acquire);
    }
    PL_CHECK(hipEventSynchronize(ctx->ev[3]));
    if (std::find(ctx->engine.begin(), ctx->engine.end(), (uint8_t)PLR_ENGINE_SEG) != ctx->engine.end()) for (int g = 0; g < SEG_MAX_GROUPS; g++) if (ctx->seg_gstream[g]) PL_CHECK(hipStreamSynchronize(ctx->seg_gstream[g]));   /* (attempts queued behind the last row: they find the images finished) */
    ctx->pending = false;
    if (seg_rc) return seg_rc;
    float ms = 0.f;
    PL_CHECK(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
    ctx->engine_ms = ms;
    PL_CHECK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[3]));
    ctx->total_ms = ms;
    if (ctx->d_records) {
        std::vector<pngloss_hip_distortion> got(ctx->n_last);
        PL_CHECK(hipMemcpy(got.data(), ctx->d_records, sizeof(pngloss_hip_distortion) * ctx->n_last, hipMemcpyDeviceToHost));
        ctx->distortion.swap(got);
    }
    if (ctx->d_ssim_records) {
        std::vector<pngloss_hip_ssim> got(ctx->n_last);
        PL_CHECK(hipMemcpy(got.data(), ctx->d_ssim_records, sizeof(pngloss_hip_ssim) * ctx->n_last, hipMemcpyDeviceToHost));
        ctx->ssim.swap(got);
    }
    int worst = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < ctx->n_last; i++) {
        int32_t r[PLR_WORDS] = { 0 };
        PL_CHECK(hipMemcpy(r, ctx->h_jobs[i].result, sizeof r, hipMemcpyDeviceToHost));
        pngloss_hip_result res;
        int32_t info[PLR_INFO_WORDS];
        pl_result_decode(r, ctx->engine[i], &res, info);
        if (results && i < n) results[i] = res;
        if (ctx->hooks.debug || ctx->hooks.segprof) print_engine_report(ctx, i, r, ctx->engine[i]);
        if (res.status) {
            std::fprintf(stderr, "pngloss_hip: image %zu: no acceptable filter row (device status %d)\n", i, res.status);
            worst = PNGLOSS_INTERNAL_ABORT;
        }
    }
    return worst;
}

namespace {

/* ---- process-wide context for the host-pointer drop-in seam ------------------------------------------------ */
std::mutex g_mu;
pngloss_hip_ctx *g_ctx = nullptr;

pngloss_hip_ctx *global_ctx()
{
    if (!g_ctx) g_ctx = pngloss_hip_create(-1);
    return g_ctx;
}

/* Upload a packed bpp-byte image as "slots" words, run, download.  rows[] may be non-contiguous. */
int run_host_image(unsigned char **rows, uint32_t width, uint32_t height, uint32_t src_bpp, uint32_t forced_bpp,
                   unsigned char *row_filters, bool verbose, unsigned strength, long bleed)
{
    if (!width || !height) return PNGLOSS_SUCCESS;
    std::lock_guard<std::mutex> lock(g_mu);
    pngloss_hip_ctx *ctx = global_ctx();
    if (!ctx) {
        std::fprintf(stderr, "pngloss_hip: no usable HIP device -- refusing to fall back to a CPU path\n");
        return PNGLOSS_HIP_ERROR;
    }
    const size_t npx = (size_t)width * height;
    std::vector<uint32_t> staging;
    try { staging.resize(npx); } catch (const std::bad_alloc &) { return PNGLOSS_OUT_OF_MEMORY_ERROR; }
    for (uint32_t y = 0; y < height; y++) pl_pack_row(staging.data() + (size_t)y * width, rows[y], width, src_bpp);
    void *d_img = nullptr, *d_filt = nullptr;
    PL_CHECK(hipSetDevice(ctx->device));
    PL_CHECK(hipMalloc(&d_img, npx * 4));
    if (row_filters) {
        hipError_t e = hipMalloc(&d_filt, height);
        if (e != hipSuccess) { (void)hipFree(d_img); return PNGLOSS_OUT_OF_MEMORY_ERROR; }
    }
    int rc = PNGLOSS_SUCCESS;
    pngloss_hip_result res{};
    do {
        if (hipMemcpy(d_img, staging.data(), npx * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = PNGLOSS_HIP_ERROR; break; }
        pngloss_hip_image_desc desc{ d_img, d_filt, width, height };
        if (verbose && !ctx->h_progress &&
            hipHostMalloc(reinterpret_cast<void **>(&ctx->h_progress), sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            ctx->h_progress = nullptr;                     /* no display then; not an error */
        if (ctx->h_progress) *ctx->h_progress = 0;
        BatchCall call{ strength, bleed, nullptr, measure_of_options(ctx) };
        call.want_progress = verbose && ctx->h_progress;
        call.sync_call = !call.want_progress;            /* (the progress display polls while the engine runs: it needs the call back at once; else the host waits anyway) */
        call.forced_bpp = forced_bpp ? &forced_bpp : nullptr;
        rc = enqueue(ctx, &desc, 1, call);
        if (rc) break;
        if (verbose && ctx->h_progress) {
            /* the progress display of pngloss_image.c:214-237: spinner at 10 Hz and the share of finished rows, on stderr */
            static const char spinner[] = "|/-\\";
            unsigned spin = 0;
            while (hipEventQuery(ctx->ev[3]) == hipErrorNotReady) {
                const uint32_t rows_done = *reinterpret_cast<volatile uint32_t *>(ctx->h_progress);
                std::fprintf(stderr, "\x1B[\x01G%c %.1f%% complete", spinner[spin++ & 3], 100.0 * rows_done / (double)height);
                std::fflush(stderr);
                std::this_thread::sleep_for(std::chrono::milliseconds(100));
            }
        }
        rc = finish(ctx, &res, 1);
        if (rc) break;
        if (hipMemcpy(staging.data(), d_img, npx * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = PNGLOSS_HIP_ERROR; break; }
        if (row_filters && hipMemcpy(row_filters, d_filt, height, hipMemcpyDeviceToHost) != hipSuccess) { rc = PNGLOSS_HIP_ERROR; break; }
    } while (0);
    (void)hipFree(d_img);
    if (d_filt) (void)hipFree(d_filt);
    if (rc == PNGLOSS_HIP_ERROR) std::fprintf(stderr, "pngloss_hip: device transfer or kernel failure: %s\n", hipGetErrorString(hipGetLastError()));
    if (rc) return rc;
    for (uint32_t y = 0; y < height; y++) pl_unpack_row(rows[y], staging.data() + (size_t)y * width, width, src_bpp);
    if (verbose) {
        /* pngloss_image.c:309-325 */
        std::fputs("\x1B[\x01G  compression complete\n", stderr);
        std::fprintf(stderr, "  used %u unique symbols\n", res.unique_symbols);
    }
    return PNGLOSS_SUCCESS;
}

/* the context that ran image `index` of the last (possibly split) host window, and the image's index there */
pngloss_hip_ctx *chunk_of(pngloss_hip_ctx *ctx, size_t &index)
{
    if (!ctx || !ctx->split_last || index < ctx->n_last) return ctx;
    for (size_t c = ctx->chunk_first.size(); c-- > 1;)
        if (index >= ctx->chunk_first[c] && c - 1 < ctx->peers.size() && ctx->peers[c - 1]) { index -= ctx->chunk_first[c]; return ctx->peers[c - 1]; }
    return ctx;
}

/* image `index` of the last batch in one of the context's per-image records (distortion, ssim, palette) ... */
template <class T> int last_record(pngloss_hip_ctx *ctx, size_t index, T *out, std::vector<T> pngloss_hip_ctx::*records)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !out || ctx->pending || index >= ctx->n_last || index >= (ctx->*records).size()) return PNGLOSS_INVALID_ARGUMENT;
    *out = (ctx->*records)[index];
    return PNGLOSS_SUCCESS;
}
/* ... and of the last call on all the GPUs of the node: in the context the image went to */
template <class T> int multi_last_record(pngloss_hip_multi *m, size_t index, T *out, std::vector<T> pngloss_hip_ctx::*records)
{
    if (!m || index >= m->where.size()) return PNGLOSS_INVALID_ARGUMENT;
    return last_record(m->ctx[(size_t)m->where[index].first], m->where[index].second, out, records);
}

} // namespace

/* ================================================================================================ C ABI */

extern "C" {

int pngloss_hip_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return -PNGLOSS_HIP_ERROR;
    return n;
}

pngloss_hip_ctx *pngloss_hip_create(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        std::fprintf(stderr, "pngloss_hip: no HIP device available\n");
        return nullptr;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= n) {
        std::fprintf(stderr, "pngloss_hip: device %d out of range (%d visible)\n", device, n);
        return nullptr;
    }
    pngloss_hip_ctx *ctx = new (std::nothrow) pngloss_hip_ctx;
    if (!ctx) return nullptr;
    ctx->device = device;
    ctx->hooks = from_env();
    { static std::atomic<int> serial{ 0 }; ctx->pin_slot = std::max(device, serial.fetch_add(1)); }
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return nullptr; }
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) { pngloss_hip_destroy(ctx); return nullptr; }
    return ctx;
}

void pngloss_hip_destroy(pngloss_hip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->seg_worker.joinable()) ctx->seg_worker.join();
    if (ctx->pending) (void)hipEventSynchronize(ctx->ev[3]);
    seg_engine_release(ctx);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (GrowBuf *b : { &ctx->d_ws, &ctx->d_arena, &ctx->h_pinned, &ctx->d_frames, &ctx->d_keep, &ctx->d_ssim, &ctx->d_target, &ctx->d_index, &ctx->d_quant }) b->release();
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->h_progress) (void)hipHostFree(ctx->h_progress);
    for (pngloss_hip_ctx *p : ctx->peers) if (p) pngloss_hip_destroy(p);
    ctx->peers.clear();
    delete ctx;
}

int pngloss_hip_optimize_batch_async(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                     unsigned quantization_strength, long bleed_divider, void *stream)
{
    return enqueue(ctx, images, n, BatchCall{ quantization_strength, bleed_divider, static_cast<hipStream_t>(stream), measure_of_options(ctx) });
}

int pngloss_hip_finish(pngloss_hip_ctx *ctx, pngloss_hip_result *results, size_t n) { return finish(ctx, results, n); }

int pngloss_hip_optimize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                               unsigned quantization_strength, long bleed_divider, void *stream,
                               pngloss_hip_result *results)
{
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    BatchCall call{ quantization_strength, bleed_divider, static_cast<hipStream_t>(stream), measure_of_options(ctx) };
    call.sync_call = call.three_groups_ok = true;
    const int rc = enqueue(ctx, images, n, call);
    if (rc) return rc;
    return finish(ctx, results, n);
}

double pngloss_hip_last_deflate_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->deflate_ms : -1.0; }
double pngloss_hip_last_engine_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->engine_ms : -1.0; }
double pngloss_hip_last_total_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->total_ms : -1.0; }

int pngloss_hip_last_histogram(pngloss_hip_ctx *ctx, size_t index, uint32_t *hist256)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !hist256 || index >= ctx->n_last || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    PL_CHECK(hipMemcpy(hist256, ctx->h_jobs[index].final_hist, sizeof(uint32_t) * PL_NSYM, hipMemcpyDeviceToHost));
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_last_original_tables(pngloss_hip_ctx *ctx, size_t index, uint32_t *freq, uint32_t *rank)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || (!freq && !rank) || index >= ctx->n_last || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    if (rank && ctx->engine[index] == PLR_ENGINE_ROWS) return PNGLOSS_INVALID_ARGUMENT;      /* (pl_rank is not run for that engine) */
    PL_CHECK(hipSetDevice(ctx->device));
    if (freq) PL_CHECK(hipMemcpy(freq, ctx->h_jobs[index].orig_hist, sizeof(uint32_t) * PL_NFILT * PL_NSYM, hipMemcpyDeviceToHost));
    if (rank) PL_CHECK(hipMemcpy(rank, ctx->h_jobs[index].orig_rank, sizeof(uint32_t) * PL_NFILT * PL_NSYM, hipMemcpyDeviceToHost));
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_last_distortion(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_distortion *out) { return last_record(ctx, index, out, &pngloss_hip_ctx::distortion); }
int pngloss_hip_last_ssim(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_ssim *out) { return last_record(ctx, index, out, &pngloss_hip_ctx::ssim); }
int pngloss_hip_last_palette(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_palette *out) { return last_record(ctx, index, out, &pngloss_hip_ctx::palette); }
int pngloss_hip_multi_last_distortion(pngloss_hip_multi *m, size_t index, pngloss_hip_distortion *out) { return multi_last_record(m, index, out, &pngloss_hip_ctx::distortion); }
int pngloss_hip_multi_last_ssim(pngloss_hip_multi *m, size_t index, pngloss_hip_ssim *out) { return multi_last_record(m, index, out, &pngloss_hip_ctx::ssim); }
int pngloss_hip_multi_last_palette(pngloss_hip_multi *m, size_t index, pngloss_hip_palette *out) { return multi_last_record(m, index, out, &pngloss_hip_ctx::palette); }
int pngloss_hip_last_index_depth(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_index_depth *out) { return last_record(ctx, index, out, &pngloss_hip_ctx::index_depth); }
int pngloss_hip_multi_last_index_depth(pngloss_hip_multi *m, size_t index, pngloss_hip_index_depth *out) { return multi_last_record(m, index, out, &pngloss_hip_ctx::index_depth); }

int pngloss_hip_last_engine_info(pngloss_hip_ctx *ctx, size_t index, int32_t info[PLR_INFO_WORDS])
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !info || index >= ctx->n_last || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    int32_t r[PLR_WORDS] = { 0 };
    PL_CHECK(hipMemcpy(r, ctx->h_jobs[index].result, sizeof r, hipMemcpyDeviceToHost));
    pngloss_hip_result res;
    pl_result_decode(r, ctx->engine[index], &res, info);
    if (ctx->engine[index] == PLR_ENGINE_SEG) { info[PLR_INFO_LAUNCH_GROUPS] = ctx->seg_groups; info[PLR_INFO_STREAM_WAIT] = ctx->seg_async_wait ? 1 : 0; }
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_set_option(pngloss_hip_ctx *ctx, const char *name, const char *value)
{
    if (!ctx || !name || !value) return PNGLOSS_INVALID_ARGUMENT;
    if (ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    /* "on" | "off" (default) into one of the caller's options */
    auto on_off = [value](bool &option) {
        const bool on = std::strcmp(value, "on") == 0;
        if (!on && std::strcmp(value, "off") != 0) return PNGLOSS_INVALID_ARGUMENT;
        option = on;
        return PNGLOSS_SUCCESS;
    };
    if (std::strcmp(name, "engine") == 0) {
        return pl_engine_pin_parse(value, &ctx->opt_engine) ? PNGLOSS_SUCCESS : PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "launch_groups") == 0) {
        /* launch groups of a large batch on the segment engine through the SYNCHRONOUS entry point: "auto" / "2" (default) or "3" -- for a process that never hands the
         * asynchronous entry a stream of its own (run_seg_engine: a third engine stream in the process halves every later engine run that waits on a caller's stream) */
        if (std::strcmp(value, "auto") == 0 || std::strcmp(value, "2") == 0) { ctx->opt_launch_groups = 0; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "3") == 0) { ctx->opt_launch_groups = 3; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "measure") == 0) {
        /* what "distortion", "ssim" and the target searches measure from here on: "all" (default) | "visible" (pl_distort_core.h, pl_ssim_core.h) */
        if (std::strcmp(value, "all") == 0) { ctx->opt_visible = false; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "visible") == 0) { ctx->opt_visible = true; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "distortion") == 0) return on_off(ctx->opt_distortion);      /* measure every batch from here on (pl_distort.hip) */
    if (std::strcmp(name, "ssim") == 0) return on_off(ctx->opt_ssim);                  /* measure the structural similarity of every batch from here on (pl_ssim.hip) */
    if (std::strcmp(name, "indexed") == 0) return on_off(ctx->opt_indexed);            /* the calls that return zlib streams also try colour type 3 from here on (pl_index.hip, window_index) */
    if (std::strcmp(name, "index_depth") == 0) {
        /* ... and with it on, at which bit depths: "8" (default) | "auto" | "min" (include/pngloss_hip_index_depth.h) */
        if (std::strcmp(value, "8") == 0) { ctx->opt_index_depth = PLI_DEPTH_8; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "auto") == 0) { ctx->opt_index_depth = PLI_DEPTH_AUTO; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "min") == 0) { ctx->opt_index_depth = PLI_DEPTH_MIN; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_INVALID_ARGUMENT;
}

int pngloss_hip_multi_set_option(pngloss_hip_multi *m, const char *name, const char *value)
{
    if (!m || m->ctx.empty()) return PNGLOSS_INVALID_ARGUMENT;
    int worst = PNGLOSS_SUCCESS;
    for (pngloss_hip_ctx *c : m->ctx) {
        const int rc = pngloss_hip_set_option(c, name, value);
        if (rc != PNGLOSS_SUCCESS) worst = rc;
    }
    return worst;
}

void *pngloss_hip_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void pngloss_hip_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

#define PL_STR2(x) #x
#define PL_STR(x) PL_STR2(x)
const char *pngloss_hip_version(void)
{
#ifdef PL_DEBUG_FORCE_FILTER
    return "pngloss_hip 0.5 DEBUGGING BUILD -DPL_DEBUG_FORCE_FILTER=" PL_STR(PL_DEBUG_FORCE_FILTER) ": one candidate wins every row, results are NOT the reference's (gfx950)";
#else
    return "pngloss_hip 0.5 (gfx950; row engines: segment-parallel v4 (units and segments from seeds, launch groups) + band-leader v2 + row statistics (strength 0); seam: pngloss_image.h:14-29)";
#endif
}

/* ---- the reference's seam ------------------------------------------------------------------------------- */

int optimize_with_rows(unsigned char **rows, uint32_t width, uint32_t height, unsigned char *row_filters,
                       bool verbose, uint_fast8_t quantization_strength, int_fast16_t bleed_divider)
{
    return run_host_image(rows, width, height, 4, 0, row_filters, verbose, quantization_strength, bleed_divider);
}

void optimize_with_stride(unsigned char *pixels, uint32_t width, uint32_t height, uint32_t stride, bool verbose,
                          uint_fast8_t quantization_strength, int_fast16_t bleed_divider)
{
    std::vector<unsigned char *> rows(height);
    for (uint32_t i = 0; i < height; i++) rows[i] = pixels + (size_t)i * stride;
    (void)optimize_with_rows(rows.data(), width, height, nullptr, verbose, quantization_strength, bleed_divider);
}

void optimizeForAverageFilter(unsigned char pixels[], int width, int height, int quantization)
{
    /* pngloss_image.c:29-38: RGBA, stride 4*w, bleed divider fixed at 2 */
    optimize_with_stride(pixels, (uint32_t)width, (uint32_t)height, (uint32_t)width * 4u, false,
                         (uint_fast8_t)quantization, 2);
}

int optimize_image(pngloss_image *image, unsigned char *row_filters, bool verbose, uint_fast8_t quantization_strength,
                   int_fast16_t bleed_divider)
{
    if (!image || image->bytes_per_pixel < 1 || image->bytes_per_pixel > 4) return PNGLOSS_INVALID_ARGUMENT;
    const uint32_t bpp = (uint32_t)image->bytes_per_pixel;
    return run_host_image(image->rows, image->width, image->height, bpp, bpp, row_filters, verbose,
                          quantization_strength, bleed_divider);
}

} /* extern "C" */

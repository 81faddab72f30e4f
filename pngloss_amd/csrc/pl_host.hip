/*
 * pl_host.hip -- the thin C-ABI shim of libpngloss_hip.so (see include/pngloss_hip.h for the contract).
 *
 * Host side only: context + workspace management, job tables, stream/event plumbing, and the host-pointer
 * drop-in entry points that replace the reference's src/pngloss_image.c:29-156.  No arithmetic of the hot path is
 * done here and there is no CPU fallback: without a usable HIP device every entry point fails loudly.  What it
 * DECIDES is in plain headers that the CPU suite pins: pl_plan.h (the batch, the segment engine's workspace table),
 * pl_seg_pace.h (the pace of the segment engine's launch thread), pl_layout.h, pl_deal.h, pl_search.h, pl_result.h.
 *
 * The context (pngloss_hip_ctx) holds what outlives a call: the caller's options (assigned by pngloss_hip_set_option and nowhere else), the buffers that
 * grow on demand (GrowBuf), streams and events, and the last batch for pngloss_hip_last_*.  What ONE call asks of a batch -- strength, stream, emit targets,
 * a synchronous caller, what to measure behind it -- is an argument (BatchCall) of enqueue: no function tells another what to run by writing into the context.
 */
#include "../../include/pngloss_hip.h"
#include "../../include/pngloss_hip_indexed.h"
#include "pl_device.h"
#include "pl_deflate.h"
#include "pl_pngread.h"
#include "pl_inflate.h"
#include "pl_distort.h"
#include "pl_ssim.h"
#include "pl_index.h"
#include "pl_target.h"
#include "pl_size.h"
#include "pl_target_dev.h"
#define SEG_PLAIN_POINTERS   /* host plumbing only: SegJob is filled here, never dereferenced */
#include "pl_seg.h"
#include "pl_plan.h"
#include "pl_seg_pace.h"
#include "pl_deal.h"
#include "pl_layout.h"
#include "pl_search.h"

#include <chrono>
#include <pthread.h>
#include <sched.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <thread>
#include <mutex>
#include <new>
#include <vector>

#define PL_CHECK(expr)                                                                                           \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            std::fprintf(stderr, "pngloss_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                                              \
            return e_ == hipErrorOutOfMemory ? PNGLOSS_OUT_OF_MEMORY_ERROR : PNGLOSS_HIP_ERROR;                  \
        }                                                                                                        \
    } while (0)

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

namespace {
/* A buffer of the context's, regrown on demand and never shrunk: device memory, or (pinned) host memory. */
struct GrowBuf {
    char *p = nullptr;
    size_t bytes = 0;
    const bool pinned;
    explicit GrowBuf(bool pinned_ = false) : pinned(pinned_) {}
    /* room for `need` bytes (pl_grow_bytes: the slack of each buffer is need / divisor); freed before the larger one is allocated, and null / 0 if that fails */
    int grow(size_t need, size_t divisor)
    {
        const size_t want = pl_grow_bytes(need, bytes, divisor);
        if (!want) return PNGLOSS_SUCCESS;
        if (p) PL_CHECK(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; bytes = 0;
        PL_CHECK(pinned ? hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void **>(&p), want));
        bytes = want;
        return PNGLOSS_SUCCESS;
    }
    void release() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
};
}

struct pngloss_hip_ctx {
    int device = 0;
    PlHooks hooks;                   /* (from the environment, at creation) */
    int pin_slot = 0;                /* which pair of CPUs of the affinity set this context's launch thread is pinned into: max(device, contexts created before it in the process) */
    int opt_launch_groups = 0;       /* pngloss_hip_set_option("launch_groups", "2" | "3" | "auto"): see run_seg_engine */
    /* one device arena, regrown on demand, carved per batch */
    GrowBuf d_ws;
    std::vector<PlJob> h_jobs;
    size_t n_last = 0;
    hipStream_t last_stream = nullptr;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; /* total start, engine start, engine stop, total stop */
    double engine_ms = -1.0, total_ms = -1.0, deflate_ms = -1.0;
    bool pending = false;
    /* host-pointer batches (pngloss_hip_optimize_batch_host*): a persistent device arena and a persistent pinned staging
     * buffer of the same layout, both regrown on demand -- no hipMalloc/hipFree and no pageable copies per call */
    GrowBuf d_arena;
    GrowBuf h_pinned{ true };
    PlEnginePin opt_engine = PlEnginePin::Auto;   /* pngloss_hip_set_option("engine", ...): Auto = the cost model (or, for tests, $PNGLOSS_HIP_ENGINE) */
    GrowBuf d_frames;                /* device frames of pngloss_hip_png_decode_batch_device: decoded RGBA8 that stays on the device for the optimiser */
    hipStream_t copy_stream = nullptr;
    double upload_ms = -1.0, download_ms = -1.0;
    /* -v progress display of the single-image seam: a host-mapped word the engine writes the finished row count to (BatchCall::want_progress) */
    uint32_t *h_progress = nullptr;
    /* segment-parallel engine: two host-mapped words (images finished, attempt being started) the control kernel writes and the
     * launch loop reads, and what the last batch did */
    bool split_last = false;         /* the last host window ran in chunks: images behind n_last are the peers' */
    std::vector<pngloss_hip_ctx *> peers;   /* further contexts on the same device: the other chunks of a host window (batch_host) */
    std::vector<size_t> chunk_first; /* first image of every chunk of the last split window (chunk 0 is this context's) */
    uint32_t *h_seg_words = nullptr;
    /* the segment engine's launch loop runs on a helper thread and on a stream of its own (the number of row attempts is decided by the
     * data): the caller's stream waits for the "images finished" word instead of for the host */
    hipStream_t seg_stream = nullptr;
    hipStream_t seg_gstream[SEG_MAX_GROUPS] = {};   /* [0] = seg_stream: one stream per GROUP of a batch's images (run_seg_engine) */
    hipEvent_t ev_seg_gdone[SEG_MAX_GROUPS] = {};
    int seg_groups = 1;
    bool seg_async_wait = false;     /* the last batch on the segment engine put a wait for the engine on the caller's stream (the asynchronous entry's non-blocking variant) */
    hipEvent_t ev_prep = nullptr;    /* caller's stream: everything the engine reads is in place */
    hipEvent_t ev_seg_done = nullptr;/* engine's stream: behind the last attempt the launch thread enqueued */
    std::thread seg_worker;
    std::atomic<int> seg_rc{ 0 };
    std::vector<SegJob> h_sj;        /* (stay alive until the asynchronous copies that read them are done: the next enqueue) */
    std::vector<uint32_t> h_sel;
    SegParams h_seg_params;
    int stream_wait_ok = -1;         /* hipStreamWaitValue32 usable on this device (-1: not asked yet) */
    int seg_prio = 0;
    bool seg_prio_distinct = false;

    /* option "distortion": the keep arena (pl_layout.h: job table, records, the originals pl_keep copies), regrown on demand like the others */
    bool opt_distortion = false;     /* pngloss_hip_set_option("distortion", "on" | "off") */
    GrowBuf d_keep;
    std::vector<PlDistortJob> h_dj;  /* (stays alive until the asynchronous copy that reads it is done: the next enqueue) */
    const PlDistortRecord *d_records = nullptr;      /* the batch in flight is measured: its records, copied back by finish */
    std::vector<pngloss_hip_distortion> distortion;  /* per image of the last finished batch; empty when it ran with the option off */

    /* option "ssim": the originals are the keep arena's (one arena, one pl_keep launch for both options); the SSIM kernel's job table and records
     * live in a small buffer of their own (pl_layout.h: pl_ssim_layout), regrown on demand like the others */
    bool opt_ssim = false;           /* pngloss_hip_set_option("ssim", "on" | "off") */
    /* option "measure": what the two measuring kernels count, behind a batch and in the probes of the target searches: every pixel, or the visible ones
     * (pl_distort_core.h, pl_ssim_core.h).  The pipeline never sees it. */
    bool opt_visible = false;        /* pngloss_hip_set_option("measure", "all" | "visible") */
    GrowBuf d_ssim;
    std::vector<PlSsimJob> h_ssj;    /* (stay alive until the asynchronous copies that read them are done: the next enqueue) */
    std::vector<PlSsimRecord> h_ssr;
    const PlSsimRecord *d_ssim_records = nullptr;    /* the batch in flight is measured: its records, copied back by finish */
    std::vector<pngloss_hip_ssim> ssim;              /* per image of the last finished batch; empty when it ran with the option off */

    /* option "indexed": the index workspace (pl_layout.h: pl_index_layout -- job table, counters, palette records, colour tables, index rows), regrown on
     * demand like the others; used by the deflate stage of a host window (window_index) */
    bool opt_indexed = false;        /* pngloss_hip_set_option("indexed", "on" | "off") */
    GrowBuf d_index;
    std::vector<pngloss_hip_palette> palette;        /* per image of the last finished host window that returned zlib streams with the option on; else empty */

    /* pngloss_hip_optimize_batch_target: the search arena (pl_target.h: tables, originals, best results so far), regrown on demand like the others */
    GrowBuf d_target;

    std::vector<uint8_t> engine;   /* per image of the last batch: the row engine its plan gave it (PLR_ENGINE_*, pl_result.h) */
    long seg_attempts = 0;
};

namespace {

/* what pl_layout.h (plain C++, no HIP) states about the device side */
static_assert(PLL_UINT4 == sizeof(uint4) && PLL_UINT2 == sizeof(uint2), "pl_layout.h: element sizes of PlJob::cand, ::err0 and ::err1");
static_assert(PLL_NFILT == PL_NFILT && PLL_NSYM == PL_NSYM && PLL_ROWSTAT_WORDS == PL_ROWSTAT_WORDS, "pl_layout.h: histogram and row counter sizes");
static_assert(PLL_FLAG_GRAY == PL_FLAG_GRAY && PLL_FLAG_OPAQUE == PL_FLAG_OPAQUE, "pl_layout.h: class flag bits");
/* the kernel's record IS the public one: finish copies it back as it stands */
static_assert(sizeof(pngloss_hip_distortion) == sizeof(PlDistortRecord) && offsetof(pngloss_hip_distortion, pixels) == offsetof(PlDistortRecord, pixels) &&
              offsetof(pngloss_hip_distortion, changed_pixels) == offsetof(PlDistortRecord, changed_pixels) && offsetof(pngloss_hip_distortion, sq_err) == offsetof(PlDistortRecord, sq_err) &&
              offsetof(pngloss_hip_distortion, max_abs) == offsetof(PlDistortRecord, max_abs), "pngloss_hip_distortion and PlDistortRecord");
static_assert(sizeof(pngloss_hip_ssim) == sizeof(PlSsimRecord) && offsetof(pngloss_hip_ssim, windows) == offsetof(PlSsimRecord, windows) &&
              offsetof(pngloss_hip_ssim, sum_q16) == offsetof(PlSsimRecord, sum_q16) && offsetof(pngloss_hip_ssim, min_q16) == offsetof(PlSsimRecord, min_q16) &&
              offsetof(pngloss_hip_ssim, reserved) == offsetof(PlSsimRecord, reserved), "pngloss_hip_ssim and PlSsimRecord");

float recip_up_host(long d)
{
    /* one ulp above the correctly rounded reciprocal: > 1/d, and far inside the exactness margin (pl_device.h) */
    float r = 1.0f / (float)d;
    r = std::nextafterf(r, 2.0f);
    return r;
}

int ensure_ws(pngloss_hip_ctx *ctx, size_t bytes) { return ctx->d_ws.grow(bytes, 4); }

/* what the device deflate (pl_deflate.h) answers, as a code of the ABI */
int deflate_rc(hipError_t e)
{
    return e == hipSuccess ? PNGLOSS_SUCCESS : e == hipErrorInvalidValue ? PNGLOSS_INVALID_ARGUMENT : e == hipErrorOutOfMemory ? PNGLOSS_OUT_OF_MEMORY_ERROR : PNGLOSS_HIP_ERROR;
}

/* The context has no "last batch" to index (pngloss_hip_last_*): enqueue begins every batch with it (only a split host window sets split_last again: batch_host) */
void forget_last_batch(pngloss_hip_ctx *c)
{
    c->n_last = 0; c->h_jobs.clear(); c->distortion.clear(); c->d_records = nullptr; c->ssim.clear(); c->d_ssim_records = nullptr; c->palette.clear(); c->split_last = false;
}
/* A search runs many batches of its own on the context: whatever happens, no "last batch" to index behind it -- for the host forms (peers), none
 * on the peers the host windows ran their other chunks on either */
struct SearchGuard {
    pngloss_hip_ctx *c; bool peers;
    ~SearchGuard() { forget_last_batch(c); if (peers) for (pngloss_hip_ctx *p : c->peers) if (p) forget_last_batch(p); }
};

struct EmitTarget { void *d_ids; void *d_rows; uint32_t pitch; };

/* What to measure behind a batch: the distortion records, the SSIM records, and whether the two count the visible pixels or all of them
 * (pl_distort_core.h, pl_ssim_core.h).  The pipeline never sees it. */
struct Measure {
    bool distortion = false, ssim = false, visible = false;
    bool indexed = false;       /* option "indexed": not a measurement, but it travels the same way -- the deflate stage of a host window (window_index) reads it, nothing else does */
};
/* ... as the caller's options ask for it: what the plain entry points hand on (no context: nothing; the call fails where it always did) */
Measure measure_of_options(const pngloss_hip_ctx *c) { return c ? Measure{ c->opt_distortion, c->opt_ssim, c->opt_visible, c->opt_indexed } : Measure{}; }

/* What one call asks of a batch (enqueue): written down by its entry point, read by enqueue and run_seg_engine, kept nowhere */
struct BatchCall {
    unsigned strength; long bleed; hipStream_t stream;
    Measure measure;
    bool sync_call = false;               /* started by a SYNCHRONOUS entry point: the caller waits on the host anyway, so its stream gets no device-side wait for the engine's finished word (run_seg_engine) */
    bool three_groups_ok = false;         /* ... and by the device-resident one itself: the batch may run as three launch groups (the host-pointer entry points, which the multi-device wrapper calls
                                             from a thread per context, stay at two: several contexts of one process share its hardware queues) */
    bool want_progress = false;           /* the engine writes image 0's finished row count to ctx->h_progress (the -v display of the single-image seam) */
    const uint32_t *forced_bpp = nullptr; /* per image, or nullptr */
    const EmitTarget *emits = nullptr;    /* per image: where its scanlines go, or nullptr */
};

/* The images `who` of a batch of host images as a batch of their own: images / lines / zs gathered into contiguous vectors (an array the caller
 * does not have stays empty and is handed on as nullptr), the results owned here; scatter puts results / lines / zs back through the same list.
 * Further per-image arrays of a call (reports, SSIM records, budgets) are its caller's, with the same list. */
struct HostSubset {
    const std::vector<size_t> &who;
    std::vector<pngloss_hip_host_image> images;
    std::vector<pngloss_hip_result> results;
    std::vector<pngloss_hip_scanlines> ln;
    std::vector<pngloss_hip_zstream> zz;
    HostSubset(const std::vector<size_t> &who_, const pngloss_hip_host_image *im, const pngloss_hip_scanlines *lines_, const pngloss_hip_zstream *zs_)
        : who(who_), images(who_.size()), results(who_.size()), ln(lines_ ? who_.size() : 0), zz(zs_ ? who_.size() : 0)
    {
        for (size_t k = 0; k < who.size(); k++) {
            images[k] = im[who[k]];
            if (lines_) ln[k] = lines_[who[k]];
            if (zs_) zz[k] = zs_[who[k]];
        }
    }
    size_t n() const { return who.size(); }
    pngloss_hip_scanlines *lines() { return ln.empty() ? nullptr : ln.data(); }
    pngloss_hip_zstream *zs() { return zz.empty() ? nullptr : zz.data(); }
    void scatter(pngloss_hip_result *results_, pngloss_hip_scanlines *lines_, pngloss_hip_zstream *zs_) const
    {
        for (size_t k = 0; k < who.size(); k++) {
            if (results_) results_[who[k]] = results[k];
            if (lines_) lines_[who[k]] = ln[k];
            if (zs_) zs_[who[k]] = zz[k];
        }
    }
};

/* The job table of a measurement into the keep arena (which the caller has grown to lay.total), its records zeroed: image i is `pixels[i]` words at img[i],
 * compared with the original at keep[i] -- or, keep == nullptr, with the place the layout gives it in the arena, for pl_keep to fill. */
int upload_distort_jobs(pngloss_hip_ctx *ctx, const PlKeepLayout &lay, size_t n, const void *const *img, const void *const *keep, const uint64_t *pixels, hipStream_t stream)
{
    PlDistortRecord *const d_rec = reinterpret_cast<PlDistortRecord *>(ctx->d_keep.p + lay.records);
    ctx->h_dj.assign(n, PlDistortJob{});
    for (size_t i = 0; i < n; i++) {
        PlDistortJob &d = ctx->h_dj[i];
        d.keep = keep ? static_cast<uint32_t *>(const_cast<void *>(keep[i])) : reinterpret_cast<uint32_t *>(ctx->d_keep.p + lay.image[i]);
        d.img = static_cast<const uint32_t *>(img[i]);
        d.pixels = pixels[i];
        d.record = d_rec + i;
    }
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

/* The segment-parallel engine on the batch in ctx->h_jobs.  All control flow of the algorithm is on the device; the host only keeps
 * a stream fed with row attempts (five kernels each, pl_seg.hip) until every image has reported that it is finished -- how many that
 * takes depends on the data.  So that the entry point stays ASYNCHRONOUS, the attempts are launched by a helper thread on a stream of
 * the context's own, at most SEG_LOOKAHEAD attempts ahead of the one the device says it is working on; the caller's stream is made
 * to wait for the host-visible "images finished" word (hipStreamWaitValue32), so everything the caller enqueues behind this call
 * still runs behind the engine.  (The images of a mixed batch that the other engine takes run on the caller's stream meanwhile.)
 * (Measured and dropped: the attempts as an executable hipGraph of 16 x (parity 0, parity 1) -- 160 kernel nodes per launch call: the
 * same engine time, and 206 - 246 ms of host CPU per 4096x4096 frame against 79 - 94 ms for the plain launches.) */
/* The engine's streams are kept for the life of the PROCESS (a free list per device): a context takes its streams from the list and gives them back when it is
 * destroyed.  Measured (round 5, tools/gpu_r5_benchlegs.sh): streams are mapped onto the process's few hardware queues when they are created; a context that
 * created fresh streams after an earlier context's three had been destroyed got two streams on ONE queue -- its two launch groups then ran one behind the other
 * (the reference's suite as one batch: 49 -> 40 Mpx/s in every bench.py run, depending on which leg came before).  Streams that are never destroyed keep their queues. */
/* process-wide: has any context put a wait for the engine on a caller's stream / does a third engine stream exist (run_seg_engine: launch groups) */
std::atomic<bool> g_stream_wait_used{ false }, g_third_engine_stream{ false };
struct SegStreamPool {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> idle;       /* (device, stream) */
    hipError_t take(int device, int prio, hipStream_t *out)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].first == device) { *out = idle[i].second; idle.erase(idle.begin() + (long)i); return hipSuccess; }
        }
        return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
    }
    void give(int device, hipStream_t s)
    {
        std::lock_guard<std::mutex> lk(mu);
        idle.insert(idle.begin(), std::make_pair(device, s));      /* (first in: the next context takes them in the order this one had them) */
    }
};
SegStreamPool &seg_stream_pool() { static SegStreamPool *p = new SegStreamPool; return *p; }      /* (never destroyed: contexts may outlive static destruction order) */

struct SegGroups { PlSegBatch b[SEG_MAX_GROUPS]; int n = 1; };
int64_t steady_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
/* The launch thread: the calls; when a group gets its next attempt, when the loop gives up and how it backs off is pl_seg_pace.h's to say. */
void seg_worker_main(pngloss_hip_ctx *ctx, SegGroups gs, long max_attempts)
{
    volatile uint32_t *words = ctx->h_seg_words;
    int rc = PNGLOSS_SUCCESS;
    if (hipSetDevice(ctx->device) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    /* Round 6: the launch thread has a CPU of its own (pl_seg_pin_cpu).  It must issue four launches every 45 - 100 us for as long as the engine runs; on a node every rank (or every
     * context of pngloss_hip_multi) has one, next to the threads that stage images.  (Measured on one box, eight contexts on one device: profiles/r06_host_side.txt: no measurable difference with 256 CPUs visible and a quota of 16 -- 181.56 against 181.62 ms for the headline frame, 1730 - 1751 against 1742 - 1796 ms for configs[3] on eight contexts of one device; all of it on TWO CPUs: 1938 ms.) */
    {
        cpu_set_t allowed;
        CPU_ZERO(&allowed);
        std::vector<int> cpus;
        if (sched_getaffinity(0, sizeof allowed, &allowed) == 0)
            for (int c = 0; c < CPU_SETSIZE; c++) if (CPU_ISSET(c, &allowed)) cpus.push_back(c);
        const int cpu = pl_seg_pin_cpu(cpus.data(), cpus.size(), ctx->pin_slot, ctx->hooks.pin);
        if (cpu >= 0) {
            cpu_set_t one;
            CPU_ZERO(&one);
            CPU_SET(cpu, &one);
            (void)pthread_setaffinity_np(pthread_self(), sizeof one, &one);       /* (a refusal is not an error: the thread stays where the scheduler puts it) */
        }
    }
    /* The engine's streams never wait for another stream ON THE DEVICE: streams share a few hardware queues, a queue is served in order,
     * and the callers' streams hold waits for the finished words -- with twelve contexts, engine j's attempts sat behind engine k's wait
     * for k's inputs, whose kernels sat behind caller j's wait for engine j.  So this thread waits for the inputs, on the host. */
    if (rc == PNGLOSS_SUCCESS && hipEventSynchronize(ctx->ev_prep) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    PlSegPace pace = pl_seg_pace_begin(gs.n, max_attempts, steady_ns());
    for (int g = 0; g < gs.n; g++) pl_seg_pace_group(pace, g, gs.b[g].n, gs.b[g].shape.seeds);
    while (rc == PNGLOSS_SUCCESS) {
        bool all_done = true, any_launched = false;
        const int64_t now = steady_ns();
        for (int g = 0; g < gs.n && rc == PNGLOSS_SUCCESS; g++) {
            const PlSegStep step = pl_seg_pace_poll(pace, g, pl_seg_words_read(words, g), now);
            if (step == PlSegStep::Finished) continue;
            all_done = false;
            if (step == PlSegStep::Busy) continue;
            if (step == PlSegStep::Runaway) {
                std::fprintf(stderr, "pngloss_hip: the segment engine needed more than %ld attempts\n", max_attempts);
                rc = PNGLOSS_HIP_ERROR;
                break;
            }
            gs.b[g].shape.seeds = pace.g[g].seeds;
            const hipError_t e = pl_seg_launch_attempt(gs.b[g], (int)pace.g[g].launched, ctx->seg_gstream[g]);
            if (e != hipSuccess) { std::fprintf(stderr, "pngloss_hip: launching a row attempt failed: %s\n", hipGetErrorString(e)); rc = PNGLOSS_HIP_ERROR; break; }
            pl_seg_pace_launched(pace, g);
            any_launched = true;
        }
        if (all_done || rc != PNGLOSS_SUCCESS) break;
        if (any_launched) continue;
        switch (pl_seg_pace_idle(pace, steady_ns())) {
        case PlSegIdle::Stalled:
            std::fprintf(stderr, "pngloss_hip: the segment engine stopped making progress (attempts of the first groups: %u %u %u %u)\n", pace.g[0].seen, pace.g[1].seen, pace.g[2].seen, pace.g[3].seen);
            rc = PNGLOSS_HIP_ERROR;
            break;
        case PlSegIdle::Yield: std::this_thread::yield(); break;
        case PlSegIdle::Sleep: std::this_thread::sleep_for(std::chrono::microseconds(100)); break;
        }
    }
    for (int g = 0; g < gs.n; g++)
        if (hipEventRecord(ctx->ev_seg_gdone[g], ctx->seg_gstream[g]) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
    if (rc != PNGLOSS_SUCCESS) {
        /* release the caller's stream, then let what is queued drain */
        for (int g = 0; g < gs.n; g++) pl_seg_words_release(words, g, gs.b[g].n);
        for (int g = 0; g < gs.n; g++) (void)hipStreamSynchronize(ctx->seg_gstream[g]);
    }
    if (ctx->hooks.debug && pace.lead_n)
        std::fprintf(stderr, "pngloss_hip: launch thread: %d group(s), %ld launches of an attempt; attempts queued ahead of the device when launching: average %.1f, least %ld, at most two ahead in %ld launches (look-ahead %ld)\n",
                     gs.n, pace.lead_n, (double)pace.lead_sum / (double)pace.lead_n, pace.lead_min, pace.lead_low, PL_SEG_LOOKAHEAD);
    ctx->seg_attempts = pl_seg_pace_attempts(pace);
    ctx->seg_rc.store(rc, std::memory_order_release);
}

int run_seg_engine(pngloss_hip_ctx *ctx, const PlJob *d_jobs, const PlPlan &plan, const PlBatchLayout &lay, const BatchCall &call,
                   const uint32_t *d_sel, const PlEngineParams &prm)
{
    const hipStream_t stream = call.stream;
    const std::vector<uint32_t> &list = plan.seg_list;
    const size_t n = list.size();                              /* the images of the batch this engine takes */
    const int ngroups = plan.ngroups;                          /* (launch groups: pl_plan_batch) */
    if (!ctx->h_seg_words) PL_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_seg_words), sizeof(uint32_t) * PL_SEG_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    if (!ctx->seg_stream) {
        /* a stream of the HIGHEST priority: streams of one priority share a few hardware queues, and a queue whose head is a caller's
         * wait for the finished word holds up everything behind it -- the engine's attempts must never sit in such a queue (twelve
         * contexts with twelve waiting streams deadlocked that way before this stream had a priority of its own) */
        int least = 0, greatest = 0;
        PL_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        ctx->seg_prio = greatest;
        PL_CHECK(seg_stream_pool().take(ctx->device, greatest, &ctx->seg_stream));
        ctx->seg_prio_distinct = greatest != least;
        ctx->seg_gstream[0] = ctx->seg_stream;
    }
    if (!ctx->ev_prep) PL_CHECK(hipEventCreateWithFlags(&ctx->ev_prep, hipEventDisableTiming));
    if (!ctx->ev_seg_done) { PL_CHECK(hipEventCreateWithFlags(&ctx->ev_seg_done, hipEventDisableTiming)); ctx->ev_seg_gdone[0] = ctx->ev_seg_done; }
    /* one stream per launch group; one launch thread feeds all of them */
    for (int g = 1; g < ngroups; g++) {
        if (!ctx->seg_gstream[g] && g >= 2) g_third_engine_stream.store(true, std::memory_order_relaxed);
        if (!ctx->seg_gstream[g]) PL_CHECK(seg_stream_pool().take(ctx->device, ctx->seg_prio, &ctx->seg_gstream[g]));
        if (!ctx->ev_seg_gdone[g]) PL_CHECK(hipEventCreateWithFlags(&ctx->ev_seg_gdone[g], hipEventDisableTiming));
    }
    ctx->seg_groups = ngroups;
    if (ctx->stream_wait_ok < 0) {
        int can = 0;
        ctx->stream_wait_ok = (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, ctx->device) == hipSuccess && can) ? 1 : 0;
        if (ctx->hooks.no_stream_wait) ctx->stream_wait_ok = 0;     /* test hook: the blocking variant */
    }
    void *d_words = nullptr;
    PL_CHECK(hipHostGetDevicePointer(&d_words, ctx->h_seg_words, 0));
    volatile uint32_t *words = ctx->h_seg_words;
    for (int q = 0; q < PL_SEG_WORDS; q++) words[q] = 0;
    uint32_t *const d_word = static_cast<uint32_t *>(d_words);
    const size_t *gfirst = plan.gfirst;
    auto group_of = [&](size_t i) { int g = 0; while (g + 1 < ngroups && i >= gfirst[g + 1]) g++; return g; };
    ctx->h_sj.assign(n, SegJob{});
    ctx->h_seg_params = plan.params;
    for (size_t i = 0; i < n; i++) {
        const PlJob &pj = ctx->h_jobs[list[i]];
        char *base = ctx->d_ws.p + lay.seg_image[i];
        SegJob &s = ctx->h_sj[i];
        s.job_index = list[i];
        s.img = pj.img; s.row_filters = pj.row_filters; s.row_ids = pj.row_ids; s.W = pj.width; s.H = pj.height; s.bpp = 0;
        s.orig_rank = pj.orig_rank; s.cand = reinterpret_cast<uint32_t *>(pj.cand);
        s.final_hist = pj.final_hist; s.result = pj.result; s.progress = pj.progress;
        const int g = group_of(i);
        s.done_counter = d_word + pl_seg_done_word(g); s.attempt_word = i == gfirst[g] ? d_word + pl_seg_attempt_word(g) : nullptr; s.break_word = d_word + pl_seg_break_word(g);
        pl_seg_bind(s, lay.seg[i], pj.width, [&](const PlSegArray &a) { return base + a.off; });
    }
    SegJob *d_sj = reinterpret_cast<SegJob *>(ctx->d_ws.p + lay.seg_jobs);
    for (size_t i = 0; i < n; i++) ctx->h_sj[i].self = d_sj + i;
    SegParams *d_params = reinterpret_cast<SegParams *>(ctx->d_ws.p + lay.seg_params);
    PL_CHECK(hipMemcpyAsync(d_sj, ctx->h_sj.data(), sizeof(SegJob) * n, hipMemcpyHostToDevice, stream));
    PL_CHECK(hipMemcpyAsync(d_params, &ctx->h_seg_params, sizeof(SegParams), hipMemcpyHostToDevice, stream));
    SegGroups gs{};
    gs.n = ngroups;
    for (int g = 0; g < ngroups; g++) {
        const PlSegGroupPlan &pg = plan.group[g];
        PlSegBatch &b = gs.b[g];
        b.d_sj = d_sj + gfirst[g]; b.d_params = d_params; b.n = pg.n; b.shape = pg;
    }
    PL_CHECK(pl_seg_launch_resolve(d_jobs, d_sj, n, stream));
    PL_CHECK(hipEventRecord(ctx->ev_prep, stream));
    if (!plan.wg_list.empty()) PL_CHECK(pl_launch_engine(d_jobs, d_sel, plan.wg_list.size(), prm, stream));      /* (a mixed batch: the other engine's images, side by side with this one's) */
    ctx->seg_rc.store(PNGLOSS_SUCCESS, std::memory_order_relaxed);
    /* (round 5, measured with tools/gpu_r5_benchlegs.sh: the stream memory operation on the caller's stream is not free -- its queue polls the finished word while
     *  the engine runs -- : without it the headline frame is 1.4 % faster, the seeded 8192 x 8192 points up to 7 %.  The synchronous entry point has no use for it.) */
    int prio = 0;
    const bool prio_known = stream && hipStreamGetPriority(stream, &prio) == hipSuccess;
    bool waiting = pl_seg_wait_on_device(ctx->stream_wait_ok != 0, ctx->seg_prio_distinct, call.sync_call, g_third_engine_stream.load(std::memory_order_relaxed), !stream, prio_known, prio, ctx->seg_prio);
    if (waiting) {
        /* the caller's stream goes on behind the engine: when every image has counted itself finished */
        for (int g = 0; g < ngroups && waiting; g++) {
            const hipError_t e = hipStreamWaitValue32(stream, d_word + pl_seg_done_word(g), (uint32_t)gs.b[g].n, hipStreamWaitValueGte, 0xFFFFFFFFu);
            if (e != hipSuccess) { (void)hipGetLastError(); ctx->stream_wait_ok = 0; waiting = false; }     /* (a wait already enqueued is satisfied when its group finishes: harmless) */
            else g_stream_wait_used.store(true, std::memory_order_relaxed);
        }
    }
    ctx->seg_async_wait = waiting;
    try { ctx->seg_worker = std::thread(seg_worker_main, ctx, gs, plan.max_attempts); }
    catch (...) { std::fprintf(stderr, "pngloss_hip: cannot start the launch thread\n"); for (int g = 0; g < ngroups; g++) pl_seg_words_release(words, g, gs.b[g].n); return PNGLOSS_HIP_ERROR; }
    if (!waiting) {
        /* no stream memory operations on this device: wait for the launch loop here, and order the caller's stream behind the engine's */
        ctx->seg_worker.join();
        for (int g = 0; g < ngroups; g++) PL_CHECK(hipStreamWaitEvent(stream, ctx->ev_seg_gdone[g], 0));
        if (ctx->seg_rc.load(std::memory_order_acquire)) return ctx->seg_rc.load();
    }
    return PNGLOSS_SUCCESS;
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

int enqueue(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const BatchCall &call)
{
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    const unsigned strength = call.strength; const long bleed = call.bleed;
    const hipStream_t stream = call.stream;
    if (strength > 255 || bleed < 1 || bleed > 32767) {
        std::fprintf(stderr, "pngloss_hip: strength must be 0..255 and bleed 1..32767 (got %u, %ld)\n", strength, bleed);
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (ctx->pending) {
        std::fprintf(stderr, "pngloss_hip: previous batch not finished; call pngloss_hip_finish first\n");
        return PNGLOSS_INVALID_ARGUMENT;
    }
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
    for (size_t i = 0; i < n; i++) {
        if (!images[i].d_rgba && images[i].width && images[i].height) return PNGLOSS_INVALID_ARGUMENT;
        in.width.push_back(images[i].width);
        in.height.push_back(images[i].height);
    }
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
    int rc = ensure_ws(ctx, lay.total);
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
    ctx->last_stream = stream;
    if (distort) ctx->d_records = reinterpret_cast<const PlDistortRecord *>(ctx->d_keep.p + keep.records);
    if (ssim) ctx->d_ssim_records = reinterpret_cast<const PlSsimRecord *>(ctx->d_ssim.p + ssim_lay.records);
    ctx->pending = true;
    return PNGLOSS_SUCCESS;
}

/* PNGLOSS_HIP_DEBUG / PNGLOSS_HIP_SEGPROF: what the row engine did for image i of the batch just finished, from its record r (pl_result.h) and the
 * engine the plan gave it.  tools/ab_*.sh grep these lines ("engine [0-9.]* ms"). */
void print_engine_report(const pngloss_hip_ctx *ctx, size_t i, const int32_t *r, int engine)
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
    /* this image's pixels (and filter flags) come back to the caller */
    bool comes_back(size_t i) const
    {
        const bool stream_only = zs && zs[i].data && (zs[i].flags & PNGLOSS_HIP_Z_STREAM_ONLY);
        return lay.im[i].px && !stream_only && results[i].status == 0;
    }
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
        if (hipMemcpy(&fl, w.ctx->h_jobs[i].out_flags, sizeof fl, hipMemcpyDeviceToHost) != hipSuccess) rc = PNGLOSS_HIP_ERROR;
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
 * kernel and nothing else, and its stream is the one the call above wrote.  Leaves the palette records of the window in ctx->palette. */
int window_index(const HostWindow &w, const std::vector<size_t> &who)
{
    pngloss_hip_ctx *ctx = w.ctx;
    pngloss_hip_zstream *zs = w.zs;
    hipStream_t stream = ctx->copy_stream;
    ctx->palette.assign(w.n, pngloss_hip_palette{});
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
    for (size_t k = 0; k < elig.size(); k++) PL_CHECK(hipMemcpyAsync(&records[k], elig[k].record, sizeof(PliRecord), hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    std::vector<pl_deflate_image> dz(elig.size());
    std::vector<std::vector<unsigned char>> out(elig.size());
    for (size_t k = 0; k < elig.size(); k++) {
        const size_t i = elig_who[k];
        if (records[k].entries != counts[i]) {
            std::fprintf(stderr, "pngloss_hip: indexed: image %zu has %u colours in its table, its counter says %u\n", i, records[k].entries, counts[i]);
            return PNGLOSS_HIP_ERROR;
        }
        out[k].resize(pl_deflate_bound((w.images[i].width + 3) / 4, w.images[i].height));      /* (the bound is stated for 4-byte pixels: width index bytes are at most that many) */
        pl_deflate_image d{};
        d.d_filter_types = elig[k].ids;
        d.d_scanlines = elig[k].rows;
        d.pitch = elig[k].pitch;
        d.rowbytes = w.images[i].width;
        d.height = w.images[i].height;
        d.out = out[k].data();
        d.out_capacity = out[k].size();
        dz[k] = d;
    }
    const int rc = deflate_rc(pl_deflate_images(dz.data(), dz.size(), nullptr));
    if (rc) return rc;
    for (size_t k = 0; k < elig.size(); k++) {
        const size_t i = elig_who[k];
        pngloss_hip_palette &p = ctx->palette[i];
        p.indexed_bytes = dz[k].out_size;
        if (!pli_keep_indexed(counts[i], p.indexed_bytes, p.truecolor_bytes, records[k].trns_entries) || dz[k].out_size > zs[i].capacity) continue;
        p.entries = records[k].entries;
        p.trns_entries = records[k].trns_entries;
        for (uint32_t e = 0; e < p.entries; e++) {
            const uint32_t word = records[k].words[e];
            p.rgb[e][0] = (uint8_t)word; p.rgb[e][1] = (uint8_t)(word >> 8); p.rgb[e][2] = (uint8_t)(word >> 16);
            p.alpha[e] = (uint8_t)(word >> 24);
        }
        std::memcpy(zs[i].data, out[k].data(), dz[k].out_size);
        zs[i].size = dz[k].out_size;
        zs[i].color_type = 3;
        zs[i].blocks[0] = dz[k].blocks_stored; zs[i].blocks[1] = dz[k].blocks_fixed; zs[i].blocks[2] = dz[k].blocks_dynamic;
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
        zs[i].size = 0; zs[i].color_type = 6; zs[i].blocks[0] = zs[i].blocks[1] = zs[i].blocks[2] = 0;
        if (!w.emits[i].pitch || w.results[i].status != 0) continue;
        uint32_t fl = 0;
        if (hipMemcpy(&fl, ctx->h_jobs[i].out_flags, sizeof fl, hipMemcpyDeviceToHost) != hipSuccess) { rc = PNGLOSS_HIP_ERROR; break; }
        zs[i].color_type = pl_color_type_of(fl);
        pl_deflate_image d{};
        d.d_filter_types = static_cast<const uint8_t *>(w.emits[i].d_ids);
        d.d_scanlines = static_cast<const uint8_t *>(w.emits[i].d_rows);
        d.pitch = w.emits[i].pitch;
        d.rowbytes = w.images[i].width * pl_emit_bpp_of(fl);
        d.height = w.images[i].height;
        d.out = zs[i].data;
        d.out_capacity = zs[i].capacity;
        dz.push_back(d);
        who.push_back(i);
    }
    if (rc == PNGLOSS_SUCCESS && !dz.empty()) {
        rc = deflate_rc(pl_deflate_images(dz.data(), dz.size(), nullptr));
        for (size_t k = 0; k < dz.size() && rc == PNGLOSS_SUCCESS; k++) {
            zs[who[k]].size = dz[k].out_size;
            zs[who[k]].blocks[0] = dz[k].blocks_stored; zs[who[k]].blocks[1] = dz[k].blocks_fixed; zs[who[k]].blocks[2] = dz[k].blocks_dynamic;
        }
    }
    if (rc == PNGLOSS_SUCCESS && w.indexed) rc = window_index(w, who);
    ctx->deflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ctx->hooks.debug_seam) std::fprintf(stderr, "pngloss_hip: host window: deflate stage %.1f ms for %zu images\n", ctx->deflate_ms, dz.size());
    return rc;
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
    for (int g = SEG_MAX_GROUPS - 1; g >= 0; g--) if (ctx->seg_gstream[g]) { (void)hipStreamSynchronize(ctx->seg_gstream[g]); seg_stream_pool().give(ctx->device, ctx->seg_gstream[g]); }   /* (back to the process's list, [0] first) */
    for (int g = 1; g < SEG_MAX_GROUPS; g++) if (ctx->ev_seg_gdone[g]) (void)hipEventDestroy(ctx->ev_seg_gdone[g]);
    if (ctx->ev_prep) (void)hipEventDestroy(ctx->ev_prep);
    if (ctx->ev_seg_done) (void)hipEventDestroy(ctx->ev_seg_done);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (GrowBuf *b : { &ctx->d_ws, &ctx->d_arena, &ctx->h_pinned, &ctx->d_frames, &ctx->d_keep, &ctx->d_ssim, &ctx->d_target, &ctx->d_index }) b->release();
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->h_progress) (void)hipHostFree(ctx->h_progress);
    if (ctx->h_seg_words) (void)hipHostFree(ctx->h_seg_words);
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

static int batch_host_one(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, unsigned quantization_strength,
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
        std::vector<uint32_t> width(n), height(n);
        for (size_t i = 0; i < n; i++) { width[i] = images[i].width; height[i] = images[i].height; }
        w.indexed = true;
        w.ilay = pl_index_layout(width, height, sizeof(PlIndexJob), sizeof(PliRecord));
        rc = ctx->d_index.grow(w.ilay.total, 8);
    }
    if (rc) return rc;
    if (!ctx->copy_stream) PL_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
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


/* A window of host images: in two halves on two contexts of the same device, a host thread each, when it is large enough -- the
 * second half is staged and uploaded while the first one computes, the first one is downloaded while the second one computes
 * (profiles/r02_host_seam.txt: staging + PCIe were 0.26 s next to a 0.28 s engine for 256 x 720p, one after the other).  The deflate
 * stage (zs) keeps its single pass: it sorts the whole window's scanlines as one stream. */
static int batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, unsigned quantization_strength,
                      long bleed_divider, Measure measure, pngloss_hip_result *results, pngloss_hip_scanlines *lines,
                      pngloss_hip_zstream *zs = nullptr)
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

int pngloss_hip_optimize_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                    unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results)
{
    return batch_host(ctx, images, n, quantization_strength, bleed_divider, measure_of_options(ctx), results, nullptr);
}

/* ---- all the GPUs of the node (replaces the one-file-at-a-time loop of /root/reference/src/pngloss.c:173-208 for a whole
 * node): one context per device, images dealt out by size (longest-processing-time first), one host thread per context,
 * results back in input order.  No collective: images are independent. ---------------------------------------------- */
struct pngloss_hip_multi {
    std::vector<pngloss_hip_ctx *> ctx;
    std::vector<std::pair<int, size_t>> where;   /* per image of the last call: the context it went to, and its index in that context's batch */
};

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

extern "C++" {       /* (templates: no C linkage) */
/* A batch of host images over the contexts of the node, the one shape of every pngloss_hip_multi_optimize_batch_host* call: the split, a host thread per
 * context that got an image, share(context, its images as a HostSubset) -> code on each, results / scanlines / streams back in input order, the codes folded
 * (pl_deal.h).  indexes_last: the call leaves a last batch per context that pngloss_hip_multi_last_* index through `where`; else `where` is cleared (the
 * searches' records are in their reports). */
template <class Share>
static int deal_over_contexts(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, pngloss_hip_result *results,
                              pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams, bool indexes_last, Share share)
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

/* One context's share of a search on host images, the one shape of both host forms.  Copies of the images go up into the search arena (laid out with the
 * SSIM tables and the scanline regions its caller names) and search(copies, layout, reports) -> code runs on them without committing; the host images stay as
 * they are until the chosen strengths run through the host-window path, once per distinct strength (pl_strength_groups) -- measured, so that every report
 * carries the record of what was written (with want_ssim the SSIM record too, into `ssim` where the caller has one; visible: both over visible pixels).  Report: .strength, .runs, .distortion.
 * empty_images_run: the rerun counts in the report of an image without pixels as well. */
template <class Report, class Search>
static int batch_host_searched(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, long bleed_divider, pngloss_hip_result *results,
                               pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, Report *reports, bool want_ssim, bool visible, pngloss_hip_ssim *ssim,
                               int scanlines, bool empty_images_run, Search search)
{
    if (!ctx || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<uint32_t> width(n), height(n), chosen(n);
    for (size_t i = 0; i < n; i++) {
        if (images[i].width && images[i].height && !images[i].rgba) return PNGLOSS_INVALID_ARGUMENT;
        width[i] = images[i].width; height[i] = images[i].height;
    }
    const PlTargetLayout lay = pl_target_layout(width, height, true, sizeof(PlMoveJob), sizeof(PlDistortJob), sizeof(PlDistortRecord),
                                                want_ssim ? sizeof(PlSsimJob) : 0, want_ssim ? sizeof(PlSsimRecord) : 0, scanlines);
    int rc = ctx->d_target.grow(lay.total, 8);
    if (rc) return rc;
    if (!ctx->copy_stream) PL_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
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
}

int pngloss_hip_multi_optimize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                          unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                          pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams)
{
    if (!m || m->ctx.empty() || (n && !images)) return PNGLOSS_INVALID_ARGUMENT;
    return deal_over_contexts(m, images, n, results, scanlines, streams, true, [&](pngloss_hip_ctx *ctx, HostSubset &mine) {
        return batch_host(ctx, mine.images.data(), mine.n(), quantization_strength, bleed_divider, measure_of_options(ctx), mine.results.data(), mine.lines(), mine.zs());
    });
}

/* ---- a strength per image, searched: pl_target.h and pl_size.h have the two rules, pl_search.h decides what is kept and which arena regions are copied
 * where, and this does what they say (include/pngloss_hip.h has the contracts) ---- */
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
        uint64_t max_pixels = 0;
        for (size_t k = 0; k < who.size(); k++) {
            const size_t i = who[k];
            dj[k].keep = reinterpret_cast<uint32_t *>(at(lay.image[i].orig));
            dj[k].img = static_cast<const uint32_t *>(images[i].d_rgba);
            dj[k].pixels = (uint64_t)images[i].width * images[i].height;
            dj[k].record = d_rec + k;
            max_pixels = std::max(max_pixels, dj[k].pixels);
        }
        PL_CHECK(hipMemcpyAsync(d_dj, dj.data(), sizeof(PlDistortJob) * dj.size(), hipMemcpyHostToDevice, stream));
        PL_CHECK(hipMemsetAsync(d_rec, 0, sizeof(PlDistortRecord) * dj.size(), stream));
        PL_CHECK(pl_launch_distort(d_dj, dj.size(), max_pixels, stream, visible));
        PL_CHECK(hipMemcpyAsync(got, d_rec, sizeof(PlDistortRecord) * dj.size(), hipMemcpyDeviceToHost, stream));
        return PNGLOSS_SUCCESS;
    }
};
}

/* images: device-resident; the arena (ctx->d_target) has been grown to lay.total.  commit: at the end every image holds the result of its chosen
 * strength (else the images are left as the last probes left them: the host form runs the chosen strengths through the host-window path). */
static int target_search(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const PlTargetLayout &lay, const pngloss_hip_target2 &t, bool visible,
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

static int target_arguments(const pngloss_hip_target2 *target, long bleed_divider)
{
    const int rc = pl_target_check2(target);
    if (rc) {
        std::fprintf(stderr, "pngloss_hip: the target needs min_psnr_db >= 0 (not NaN), max_abs_error 0..255, max_strength 0..255 and min_ssim 0..1 (not NaN)\n");
        return rc;
    }
    if (bleed_divider < 1 || bleed_divider > 32767) {
        std::fprintf(stderr, "pngloss_hip: bleed must be 1..32767 (got %ld)\n", bleed_divider);
        return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_SUCCESS;
}

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
    if (ctx->pending) {
        std::fprintf(stderr, "pngloss_hip: previous batch not finished; call pngloss_hip_finish first\n");
        return PNGLOSS_INVALID_ARGUMENT;
    }
    std::vector<uint32_t> width(n), height(n);
    for (size_t i = 0; i < n; i++) {
        if (!images[i].d_rgba && images[i].width && images[i].height) return PNGLOSS_INVALID_ARGUMENT;
        width[i] = images[i].width; height[i] = images[i].height;
    }
    PL_CHECK(hipSetDevice(ctx->device));
    /* room for every original and every best result beside the workspace -- or the call fails here, with no image touched */
    const bool want_ssim = target->min_ssim != 0.0;
    const PlTargetLayout lay = pl_target_layout(width, height, false, sizeof(PlMoveJob), sizeof(PlDistortJob), sizeof(PlDistortRecord),
                                                want_ssim ? sizeof(PlSsimJob) : 0, want_ssim ? sizeof(PlSsimRecord) : 0);
    rc = ctx->d_target.grow(lay.total, 8);
    if (rc) return rc;
    return target_search(ctx, images, n, lay, *target, ctx->opt_visible, bleed_divider, static_cast<hipStream_t>(stream), true, results, reports, ssim);
}

/* one context's share of pngloss_hip_multi_optimize_batch_host_target: the rerun of the chosen strength counts for every image */
static int batch_host_target(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_target2 &target, long bleed_divider,
                             pngloss_hip_result *results, pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, pngloss_hip_target_report *reports,
                             pngloss_hip_ssim *ssim)
{
    const bool visible = measure_of_options(ctx).visible;      /* option "measure": for the probes and for the records of the reruns */
    return batch_host_searched(ctx, images, n, bleed_divider, results, lines, zs, reports, target.min_ssim != 0.0, visible, ssim, PLT_SCANLINES_OFF, true,
                               [&](const pngloss_hip_image_desc *copies, const PlTargetLayout &lay, pngloss_hip_target_report *rep) {
                                   return target_search(ctx, copies, n, lay, target, visible, bleed_divider, ctx->copy_stream, false, nullptr, rep, nullptr);
                               });
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

/* ---- a strength per image from a byte budget: pl_size.h has the rule, pl_search.h the bookkeeping (SearchDevice: in front of target_search) ---- */
/* images: device-resident; the arena (ctx->d_target) has been grown to lay.total, laid out with a scanline region (and, with `streams`, the best
 * result's).  commit: at the end every image holds the result of its chosen strength and `streams` (may be nullptr) are written; else the images are
 * left as the last probes left them (the host form runs the chosen strengths through the host-window path). */
static int size_search(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const PlTargetLayout &lay, const pngloss_hip_size_target &t,
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
    /* what the deflate is to look at: image i's scanlines in the probe region or in the stash, in the colour type `flags` says */
    auto deflate_image = [&](size_t i, bool stash, uint32_t flags) {
        pl_deflate_image d{};
        d.d_filter_types = static_cast<const uint8_t *>(dev.address((uint32_t)i, stash ? PLA_BEST_IDS : PLA_IDS));
        d.d_scanlines = static_cast<const uint8_t *>(dev.address((uint32_t)i, stash ? PLA_BEST_ROWS : PLA_ROWS));
        d.pitch = lay.image[i].pitch;
        d.rowbytes = images[i].width * pl_emit_bpp_of(flags);
        d.height = images[i].height;
        return d;
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
            if (st[i].last.result.status == 0) { dz.push_back(deflate_image(i, false, st[i].last.flags)); measured.push_back(i); }
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
            streams[i].size = 0; streams[i].color_type = 6; streams[i].blocks[0] = streams[i].blocks[1] = streams[i].blocks[2] = 0;
            if (!has_pixels(i) || st[i].kept.result.status != 0) continue;
            streams[i].color_type = pl_color_type_of(st[i].kept.flags);
            pl_deflate_image d = deflate_image(i, st[i].kept_in_stash, st[i].kept.flags);
            d.out = streams[i].data;
            d.out_capacity = streams[i].capacity;
            dz.push_back(d);
            who.push_back(i);
        }
        if (!dz.empty()) {
            rc = deflate_rc(pl_deflate_images(dz.data(), dz.size(), stream));
            if (rc) return rc;
        }
        for (size_t k = 0; k < dz.size(); k++) {
            pngloss_hip_zstream &z = streams[who[k]];
            z.size = dz[k].out_size;
            z.blocks[0] = dz[k].blocks_stored; z.blocks[1] = dz[k].blocks_fixed; z.blocks[2] = dz[k].blocks_dynamic;
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

static int size_arguments(const pngloss_hip_size_target *target, size_t n, const uint32_t *width, const uint32_t *height, long bleed_divider)
{
    const int rc = pl_size_check(target, n, width, height);
    if (rc) {
        std::fprintf(stderr, "pngloss_hip: the size target needs max_strength 0..255, a budget above 0 for every image that has pixels, and images of at most 1 GiB of scanlines\n");
        return rc;
    }
    if (bleed_divider < 1 || bleed_divider > 32767) {
        std::fprintf(stderr, "pngloss_hip: bleed must be 1..32767 (got %ld)\n", bleed_divider);
        return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_optimize_batch_size(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                    const pngloss_hip_size_target *target, long bleed_divider, void *stream,
                                    pngloss_hip_result *results, pngloss_hip_zstream *streams, pngloss_hip_size_report *reports)
{
    if (n && !images) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<uint32_t> width(n), height(n);
    for (size_t i = 0; i < n; i++) { width[i] = images[i].width; height[i] = images[i].height; }
    int rc = size_arguments(target, n, width.data(), height.data(), bleed_divider);
    if (rc) return rc;
    if (!ctx) return PNGLOSS_INVALID_ARGUMENT;
    if (ctx->pending) {
        std::fprintf(stderr, "pngloss_hip: previous batch not finished; call pngloss_hip_finish first\n");
        return PNGLOSS_INVALID_ARGUMENT;
    }
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

/* one context's share of pngloss_hip_multi_optimize_batch_host_size: no SSIM, scanline regions for the probes, and the rerun of the chosen strength counts
 * only for an image that has pixels (one without ends with 0 runs) */
static int batch_host_size(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_size_target &target, long bleed_divider,
                           pngloss_hip_result *results, pngloss_hip_scanlines *lines, pngloss_hip_zstream *zs, pngloss_hip_size_report *reports)
{
    /* the byte budget reports over all pixels, whatever the option "measure" says */
    return batch_host_searched(ctx, images, n, bleed_divider, results, lines, zs, reports, false, false, nullptr, PLT_SCANLINES_PROBE, false,
                               [&](const pngloss_hip_image_desc *copies, const PlTargetLayout &lay, pngloss_hip_size_report *rep) {
                                   return size_search(ctx, copies, n, lay, target, bleed_divider, ctx->copy_stream, false, nullptr, nullptr, rep);
                               });
}

int pngloss_hip_multi_optimize_batch_host_size(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n,
                                               const pngloss_hip_size_target *target, long bleed_divider, pngloss_hip_result *results,
                                               pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                               pngloss_hip_size_report *reports)
{
    if (n && !images) return PNGLOSS_INVALID_ARGUMENT;
    {
        std::vector<uint32_t> width(n), height(n);
        for (size_t i = 0; i < n; i++) { width[i] = images[i].width; height[i] = images[i].height; }
        const int arc = size_arguments(target, n, width.data(), height.data(), bleed_divider);
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
double pngloss_hip_last_deflate_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->deflate_ms : -1.0; }

double pngloss_hip_last_engine_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->engine_ms : -1.0; }
double pngloss_hip_last_total_ms(const pngloss_hip_ctx *ctx) { return ctx ? ctx->total_ms : -1.0; }

/* the context that ran image `index` of the last (possibly split) host window, and the image's index there */
static pngloss_hip_ctx *chunk_of(pngloss_hip_ctx *ctx, size_t &index)
{
    if (!ctx || !ctx->split_last || index < ctx->n_last) return ctx;
    for (size_t c = ctx->chunk_first.size(); c-- > 1;)
        if (index >= ctx->chunk_first[c] && c - 1 < ctx->peers.size() && ctx->peers[c - 1]) { index -= ctx->chunk_first[c]; return ctx->peers[c - 1]; }
    return ctx;
}

int pngloss_hip_last_histogram(pngloss_hip_ctx *ctx, size_t index, uint32_t *hist256)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !hist256 || index >= ctx->n_last || ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
    PL_CHECK(hipSetDevice(ctx->device));
    PL_CHECK(hipMemcpy(hist256, ctx->h_jobs[index].final_hist, sizeof(uint32_t) * PL_NSYM, hipMemcpyDeviceToHost));
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_last_distortion(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_distortion *out)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !out || ctx->pending || index >= ctx->n_last || index >= ctx->distortion.size()) return PNGLOSS_INVALID_ARGUMENT;
    *out = ctx->distortion[index];
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_multi_last_distortion(pngloss_hip_multi *m, size_t index, pngloss_hip_distortion *out)
{
    if (!m || index >= m->where.size()) return PNGLOSS_INVALID_ARGUMENT;
    return pngloss_hip_last_distortion(m->ctx[(size_t)m->where[index].first], m->where[index].second, out);
}

int pngloss_hip_last_ssim(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_ssim *out)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !out || ctx->pending || index >= ctx->n_last || index >= ctx->ssim.size()) return PNGLOSS_INVALID_ARGUMENT;
    *out = ctx->ssim[index];
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_multi_last_ssim(pngloss_hip_multi *m, size_t index, pngloss_hip_ssim *out)
{
    if (!m || index >= m->where.size()) return PNGLOSS_INVALID_ARGUMENT;
    return pngloss_hip_last_ssim(m->ctx[(size_t)m->where[index].first], m->where[index].second, out);
}

int pngloss_hip_last_palette(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_palette *out)
{
    ctx = chunk_of(ctx, index);
    if (!ctx || !out || ctx->pending || index >= ctx->n_last || index >= ctx->palette.size()) return PNGLOSS_INVALID_ARGUMENT;
    *out = ctx->palette[index];
    return PNGLOSS_SUCCESS;
}

int pngloss_hip_multi_last_palette(pngloss_hip_multi *m, size_t index, pngloss_hip_palette *out)
{
    if (!m || index >= m->where.size()) return PNGLOSS_INVALID_ARGUMENT;
    return pngloss_hip_last_palette(m->ctx[(size_t)m->where[index].first], m->where[index].second, out);
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
    std::vector<uint32_t> width(n), height(n);
    for (size_t i = 0; i < n; i++) {
        if (pairs[i].width && pairs[i].height && (!pairs[i].d_a || !pairs[i].d_b)) return PNGLOSS_INVALID_ARGUMENT;
        a[i] = pairs[i].d_a; b[i] = pairs[i].d_b;
        width[i] = pairs[i].width; height[i] = pairs[i].height;
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

static bool compare_refused(pngloss_hip_ctx *ctx)
{
    if (!ctx->pending) return false;
    std::fprintf(stderr, "pngloss_hip: a batch is in flight on this context; call pngloss_hip_finish first\n");
    return true;
}

int pngloss_hip_compare_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out, void *stream_)
{
    if (!ctx || (n && (!pairs || !out))) return PNGLOSS_INVALID_ARGUMENT;
    if (compare_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    return compare_distortion(ctx, pairs, n, out, static_cast<hipStream_t>(stream_), false);
}

int pngloss_hip_compare_batch_ssim(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_ssim *out, void *stream_)
{
    if (!ctx || (n && (!pairs || !out))) return PNGLOSS_INVALID_ARGUMENT;
    if (compare_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
    if (!n) return PNGLOSS_SUCCESS;
    return compare_ssim(ctx, pairs, n, out, static_cast<hipStream_t>(stream_), false);
}

int pngloss_hip_compare_batch_visible(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out_distortion,
                                      pngloss_hip_ssim *out_ssim, void *stream_)
{
    if (!ctx || (n && !pairs)) return PNGLOSS_INVALID_ARGUMENT;
    if (compare_refused(ctx)) return PNGLOSS_INVALID_ARGUMENT;
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

int pngloss_hip_png_decode_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n)
{
    return pngloss_hip_png_decode_batch_host_status(ctx, src, n, nullptr);
}

} /* extern "C" */
/* `interlace` sits where both source structs had padding: their size and every other member's offset are what they were before it */
static_assert(sizeof(pngloss_hip_png_source) == 64 && offsetof(pngloss_hip_png_source, interlace) == 18 && offsetof(pngloss_hip_png_source, palette) == 24 &&
              offsetof(pngloss_hip_png_source, palette_entries) == 32 && offsetof(pngloss_hip_png_source, trns) == 40 &&
              offsetof(pngloss_hip_png_source, trns_bytes) == 48 && offsetof(pngloss_hip_png_source, rgba) == 56, "pngloss_hip_png_source layout");
static_assert(sizeof(pngloss_hip_png_zsource) == 64 && offsetof(pngloss_hip_png_zsource, interlace) == 26 && offsetof(pngloss_hip_png_zsource, palette) == 32 &&
              offsetof(pngloss_hip_png_zsource, palette_entries) == 40 && offsetof(pngloss_hip_png_zsource, trns) == 48 &&
              offsetof(pngloss_hip_png_zsource, trns_bytes) == 56, "pngloss_hip_png_zsource layout");
namespace {
/* d_out == nullptr: the decoded images are downloaded to src[i].rgba.  Else they STAY on the device, in the context's frame arena (apart
 * from the workspace the optimiser carves up), and d_out[i] receives their device pointers. */
/* zs != nullptr: src[i].scanlines is not used; the scanlines are INFLATED ON THE DEVICE from zs[i] (the concatenated IDAT payloads), one wave per file */
struct ZRef { const unsigned char *z; size_t bytes; };
/* per_image: set once the batch as a whole went through -- from there on the return value is the worst PER-IMAGE status and status[] explains it.
 * A return before that point is a failure of the WHOLE batch (bad argument, allocation, copy, launch, device fault): png_decode_common then
 * writes that code into every status[i], so that a caller who looks at status[] alone never takes an undecoded image for a decoded one. */
int png_decode_body(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status, void **d_out, hipStream_t stream, const ZRef *zs, bool &per_image)
{
    if (!ctx || (!src && n)) return PNGLOSS_INVALID_ARGUMENT;
    if (status) for (size_t i = 0; i < n; i++) status[i] = PNGLOSS_SUCCESS;
    if (d_out) for (size_t i = 0; i < n; i++) d_out[i] = nullptr;
    if (!n) { per_image = true; return PNGLOSS_SUCCESS; }
    if (ctx->pending) {
        /* (the workspace this call carves up belongs to the batch in flight) */
        std::fprintf(stderr, "pngloss_hip: a batch is in flight on this context; call pngloss_hip_finish first\n");
        return PNGLOSS_INVALID_ARGUMENT;
    }
    PL_CHECK(hipSetDevice(ctx->device));
    std::vector<PrFormat> fmt(n);
    std::vector<PlReadIn> in(n);
    static const unsigned char bad_stream[6] = { 0, 0, 0, 0, 0, 0 };       /* (CMF 0: not deflate) */
    std::vector<ZRef> zsub(zs ? n : 0);
    for (size_t i = 0; i < n; i++) {
        if ((!zs && !src[i].scanlines) || (zs && !zs[i].z) || (!d_out && !src[i].rgba)) return PNGLOSS_INVALID_ARGUMENT;
        if (src[i].interlace > 1) {
            std::fprintf(stderr, "pngloss_hip: image %zu: interlace method %d (0 = none, 1 = Adam7; the struct has to be zero-initialised)\n", i, src[i].interlace);
            return PNGLOSS_INVALID_ARGUMENT;
        }
        /* a stream too short to be zlib's (header + one block + Adler-32) or beyond the inflater's 32-bit positions is THAT file's problem: it gets
         * status 25 like any other stream the inflater refuses (it is handed a six-byte stream with an invalid header), the batch goes on */
        if (zs && (zs[i].bytes < 6 || zs[i].bytes > 0xFFFFFFF0u)) zsub[i] = ZRef{ bad_stream, sizeof bad_stream };
        else if (zs) zsub[i] = zs[i];
        PrFormat &F = fmt[i];
        if (!pr_format(F, src[i].width, src[i].height, src[i].color_type, src[i].bit_depth, src[i].palette, src[i].palette_entries, src[i].trns, src[i].trns_bytes)) {
            std::fprintf(stderr, "pngloss_hip: image %zu: colour type %d with bit depth %d (or an empty image / a palette image without PLTE) is not a PNG format\n", i, src[i].color_type, src[i].bit_depth);
            return PNGLOSS_INVALID_ARGUMENT;
        }
        if (zs && pr_scanline_bytes(F.width, F.height, F.color_type, F.bit_depth, src[i].interlace) > 0xFFFFFFF0u) return PNGLOSS_INVALID_ARGUMENT;     /* (32-bit positions in the inflater) */
        in[i] = PlReadIn{ F.width, F.height, F.color_type, F.bit_depth, src[i].interlace, zs ? (uint64_t)zsub[i].bytes : PL_READ_NO_STREAM };
    }
    /* where everything lies (pl_layout.h): the tables in front -- jobs, then the status words of the decode and of the inflate and the progress words
     * (zeroed by one memset), then the inflate's streams --, the files' data behind them.  (Every job carries its format, palette included: 1.1 KB a
     * pass.  A first version whose jobs pointed at one format per file had a table 4.6 MB smaller at 768 interlaced files, but a kernel 13 % slower
     * on plain files: DESIGN.md section 9.2) */
    const PlReadLayout lay = pl_read_layout(in, d_out != nullptr, sizeof(PrJob), sizeof(PliStream));
    const size_t m = lay.job.size(), total = lay.total, ftotal = lay.ftotal;
    const auto tr0 = std::chrono::steady_clock::now();
    auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(); };
    int rc = ensure_ws(ctx, total);
    if (rc == PNGLOSS_SUCCESS && d_out) rc = ctx->d_frames.grow(ftotal, 4);
    if (rc) return rc;
    const double ms_ws = ms_since();
    /* offsets into pointers: here and nowhere else */
    char *const b = ctx->d_ws.p, *const fb = d_out ? ctx->d_frames.p : b;
    int32_t *d_status = reinterpret_cast<int32_t *>(b + lay.status), *d_zstatus = reinterpret_cast<int32_t *>(b + lay.zstatus);
    uint32_t *d_prog = reinterpret_cast<uint32_t *>(b + lay.prog);
    PliStream *d_zjobs = reinterpret_cast<PliStream *>(b + lay.zjobs);
    auto d_raw = [&](size_t i) { return reinterpret_cast<uint8_t *>(b + lay.file[i].raw); };
    auto d_z = [&](size_t i) { return reinterpret_cast<uint8_t *>(b + lay.file[i].z); };
    auto d_rgba = [&](size_t i) { return fb + lay.file[i].out; };
    std::vector<PrJob> jobs(m);
    for (size_t k = 0; k < m; k++) {
        const PlReadJob &a = lay.job[k];
        PrJob &j = jobs[k];
        j.F = fmt[a.file];                                                    /* (a pass: the file's format with the pass's geometry) */
        j.F.width = a.width; j.F.height = a.height; j.F.rowbytes = a.rowbytes;
        j.ox = a.ox; j.oy = a.oy; j.sx = a.sx; j.sy = a.sy; j.pitch = a.pitch;
        j.nbands = a.nbands; j.lastpitch = a.lastpitch;
        j.raw = reinterpret_cast<const uint8_t *>(b + a.raw);
        j.rgba = reinterpret_cast<uint32_t *>(d_rgba(a.file));
        j.lastrow = reinterpret_cast<uint8_t *>(b + a.last);
        j.progress = d_prog + a.prog;
        j.status = d_status + a.file;
    }
    std::vector<PliStream> zjobs(zs ? n : 0);
    PL_CHECK(hipMemsetAsync(d_status, 0, lay.zeroed, stream));
    for (size_t i = 0; i < n; i++) {
        /* (from pinned memory -- pngloss_hip_pinned_alloc -- this is one DMA; from pageable memory the runtime stages it: 33 ms against 1.3 for 64 MiB) */
        if (zs) {
            PL_CHECK(hipMemcpyAsync(d_z(i), zsub[i].z, zsub[i].bytes, hipMemcpyHostToDevice, stream));
            zjobs[i].z = d_z(i); zjobs[i].zbytes = (uint32_t)zsub[i].bytes;
            zjobs[i].out = d_raw(i); zjobs[i].expect = (uint32_t)lay.file[i].raw_bytes;
            zjobs[i].status = d_zstatus + i;
        } else
        PL_CHECK(hipMemcpyAsync(d_raw(i), src[i].scanlines, lay.file[i].raw_bytes, hipMemcpyHostToDevice, stream));
    }
    PL_CHECK(hipMemcpyAsync(b, jobs.data(), sizeof(PrJob) * m, hipMemcpyHostToDevice, stream));
    if (zs) {
        PL_CHECK(hipMemcpyAsync(d_zjobs, zjobs.data(), sizeof(PliStream) * n, hipMemcpyHostToDevice, stream));
        PL_CHECK(pl_launch_inflate(d_zjobs, n, stream));
    }
    const bool seam_dbg = ctx->hooks.debug_seam;
    double ms_up = 0, ms_k = 0;
    if (seam_dbg) { PL_CHECK(hipStreamSynchronize(stream)); ms_up = ms_since(); }
    PL_CHECK(pl_launch_png_decode(reinterpret_cast<const PrJob *>(b), m, lay.max_bands, stream));
    if (seam_dbg) { PL_CHECK(hipStreamSynchronize(stream)); ms_k = ms_since(); }
    std::vector<int32_t> st(n), zst(n, 0);
    if (zs) PL_CHECK(hipMemcpyAsync(zst.data(), d_zstatus, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    if (!d_out)
        for (size_t i = 0; i < n; i++)
            PL_CHECK(hipMemcpyAsync(src[i].rgba, d_rgba(i), (size_t)src[i].width * src[i].height * 4, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipMemcpyAsync(st.data(), d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    PL_CHECK(hipStreamSynchronize(stream));
    if (seam_dbg) std::fprintf(stderr, "pngloss_hip: read side: %zu files, workspace %zu MB ready after %.1f ms, upload %.1f ms, unfilter + expand %.1f ms, %s %.1f ms\n", n, (total + ftotal) >> 20, ms_ws, ms_up - ms_ws, ms_k - ms_up, d_out ? "status (the frames stay on the device)" : "download", ms_since() - ms_k);
    /* every image has been decoded (and downloaded); the ones that failed say so -- one damaged file does not take the window with it */
    per_image = true;
    int worst = PNGLOSS_SUCCESS;
    for (size_t i = 0; i < n; i++) {
        if (d_out) d_out[i] = d_rgba(i);
        if (zst[i]) {
            /* the stream is not one the device inflater takes (damaged, or beyond what it checks): the caller reads the file on the host */
            std::fprintf(stderr, "pngloss_hip: image %zu: the device inflater stopped (code %d): corrupt or unusual zlib stream\n", i, zst[i]);
            if (status) status[i] = 25;
            if (worst == PNGLOSS_SUCCESS) worst = 25;
            continue;
        }
        if (!st[i]) continue;
        const int code = st[i] == 25 ? 25 : PNGLOSS_HIP_ERROR;
        if (st[i] == 25) std::fprintf(stderr, "pngloss_hip: image %zu: a scanline has a filter type beyond 4 (corrupt stream)\n", i);
        else std::fprintf(stderr, "pngloss_hip: image %zu: the row bands of the decoder lost step (internal error %d)\n", i, st[i]);
        if (status) status[i] = code;
        if (worst == PNGLOSS_SUCCESS || code == PNGLOSS_HIP_ERROR) worst = code;
    }
    return worst;
}
int png_decode_common(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status, void **d_out, hipStream_t stream, const ZRef *zs = nullptr)
{
    bool per_image = false;
    const int rc = png_decode_body(ctx, src, n, status, d_out, stream, zs, per_image);
    if (!per_image && rc != PNGLOSS_SUCCESS) {
        /* the batch as a whole failed: nothing in rgba / d_out is a decoded image */
        if (status) for (size_t i = 0; i < n; i++) status[i] = rc;
        if (d_out) for (size_t i = 0; i < n; i++) d_out[i] = nullptr;
    }
    return rc;
}
} // namespace
extern "C" {

int pngloss_hip_png_decode_batch_host_status(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status)
{
    return png_decode_common(ctx, src, n, status, nullptr, nullptr);
}

int pngloss_hip_png_decode_batch_device(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, void **d_rgba, int *status, void *stream)
{
    if (!d_rgba && n) return PNGLOSS_INVALID_ARGUMENT;
    return png_decode_common(ctx, src, n, status, d_rgba, static_cast<hipStream_t>(stream));
}

int pngloss_hip_png_decode_batch_device_z(pngloss_hip_ctx *ctx, const pngloss_hip_png_zsource *zsrc, size_t n, void **d_rgba, int *status, void *stream)
{
    if ((!d_rgba || !zsrc) && n) return PNGLOSS_INVALID_ARGUMENT;
    std::vector<pngloss_hip_png_source> src(n);
    std::vector<ZRef> zs(n);
    for (size_t i = 0; i < n; i++) {
        src[i] = pngloss_hip_png_source{ nullptr, zsrc[i].width, zsrc[i].height, zsrc[i].color_type, zsrc[i].bit_depth, zsrc[i].interlace, zsrc[i].palette, zsrc[i].palette_entries, zsrc[i].trns, zsrc[i].trns_bytes, nullptr };
        zs[i] = ZRef{ zsrc[i].zstream, zsrc[i].zbytes };
    }
    return png_decode_common(ctx, src.data(), n, status, d_rgba, static_cast<hipStream_t>(stream), zs.data());
}

int pngloss_hip_set_option(pngloss_hip_ctx *ctx, const char *name, const char *value)
{
    if (!ctx || !name || !value) return PNGLOSS_INVALID_ARGUMENT;
    if (ctx->pending) return PNGLOSS_INVALID_ARGUMENT;
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
    if (std::strcmp(name, "distortion") == 0) {
        /* measure every batch from here on (pl_distort.hip): "on" | "off" (default) */
        if (std::strcmp(value, "on") == 0) { ctx->opt_distortion = true; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "off") == 0) { ctx->opt_distortion = false; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "measure") == 0) {
        /* what "distortion", "ssim" and the target searches measure from here on: "all" (default) | "visible" (pl_distort_core.h, pl_ssim_core.h) */
        if (std::strcmp(value, "all") == 0) { ctx->opt_visible = false; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "visible") == 0) { ctx->opt_visible = true; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "indexed") == 0) {
        /* the calls that return zlib streams also try colour type 3 from here on (pl_index.hip, window_index): "on" | "off" (default) */
        if (std::strcmp(value, "on") == 0) { ctx->opt_indexed = true; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "off") == 0) { ctx->opt_indexed = false; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    if (std::strcmp(name, "ssim") == 0) {
        /* measure the structural similarity of every batch from here on (pl_ssim.hip): "on" | "off" (default) */
        if (std::strcmp(value, "on") == 0) { ctx->opt_ssim = true; return PNGLOSS_SUCCESS; }
        if (std::strcmp(value, "off") == 0) { ctx->opt_ssim = false; return PNGLOSS_SUCCESS; }
        return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_INVALID_ARGUMENT;
}

void *pngloss_hip_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void pngloss_hip_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

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

/*
 * pl_host_ctx.h -- PRIVATE to the host shim of libpngloss_hip.so (the pl_host*.hip files; not installed under include/): the context, what one call
 * hands to a batch, and the few functions that cross a file boundary.
 *
 * The map of the host side -- one concern per file, and no kernel in any of them:
 *   pl_host.hip          the context's life (create / destroy, the environment's hooks, the options), the batch pipeline (enqueue, finish, the engine
 *                        report, the cost model's calibration), the plain optimize_batch* entry points, pngloss_hip_last_*, the single-image seam
 *   pl_host_seg.hip      the segment engine: its process-wide stream pool, its launch thread, run_seg_engine
 *   pl_host_window.hip   a window of host images and its stages (stage, upload, download, scanlines, deflate / indexed), the split over contexts of
 *                        one device (batch_host), the multi-GPU object and its dealer, the *_batch_host* entry points
 *   pl_host_search.hip   the two strength searches (target_search, size_search), their host form and their entry points
 *   pl_host_measure.hip  the job tables of the two measuring kernels, the stand-alone comparisons
 *   pl_host_read.hip     the PNG read side
 *   pl_host_quant.hip    the colour quantiser: its workspace, the median cut between its two synchronisations, its host form -- with and without the dither pass (pl_dither.hip)
 *   pl_host_quant_target.hip  the colour count searched per image from a distortion target (pl_colors.h), over the stages of pl_host_quant.hip
 *   pl_host_quant_space.hip   the entry points that name the space the palette search runs in (include/pngloss_hip_quant_space.h): they split
 *                        the parameter record and call what the older entry points of the two files above call
 * What the host side DECIDES is in plain headers that the CPU suite pins (pl_plan.h, pl_seg_pace.h, pl_layout.h, pl_deal.h, pl_search.h, pl_result.h);
 * these files carry it out.
 *
 * WHO WRITES WHAT.  The members of pngloss_hip_ctx stand in blocks, one per file, and a member is written by the file its block names and by no
 * other.  The exceptions, all of them:
 *   - pngloss_hip_destroy (pl_host.hip) frees what every block holds (the engine's part through seg_engine_release).
 *   - forget_last_batch (pl_host.hip) clears every block's record of the last batch; enqueue begins with it, the searches end with it.
 *   - pl_host.hip joins the launch thread (seg_worker) and synchronises the engine's streams where a batch ends: enqueue, finish, destroy.
 *   - a buffer is grown by whoever lays it out: d_ws by enqueue and by the read side, d_keep by enqueue and by the comparisons.
 *   - the quantiser's host form makes sure of copy_stream (ensure_copy_stream), as the searches do.
 *   - batch_host (pl_host_window.hip) folds the peers' times into engine_ms and total_ms of the context it was called on.
 *   - engine_calib (pl_host.hip) pins opt_engine on the temporary context it measures with.
 * Every file may READ every member.  What ONE call asks of a batch is never a member: it is a BatchCall, an argument of enqueue.
 */
#ifndef PL_HOST_CTX_H
#define PL_HOST_CTX_H

#include "../../include/pngloss_hip.h"
#include "../../include/pngloss_hip_indexed.h"
#include "../../include/pngloss_hip_index_depth.h"
#include "../../include/pngloss_hip_quant.h"
#include "../../include/pngloss_hip_dither.h"
#include "../../include/pngloss_hip_quant_target.h"
#include "../../include/pngloss_hip_quant_space.h"
#include "pl_device.h"
#include "pl_deflate.h"
#include "pl_pngread.h"
#include "pl_inflate.h"
#include "pl_distort.h"
#include "pl_ssim.h"
#include "pl_index.h"
#include "pl_quant.h"
#include "pl_dither.h"
#include "pl_target.h"
#include "pl_size.h"
#include "pl_colors.h"
#include "pl_target_dev.h"
#define SEG_PLAIN_POINTERS   /* host plumbing only: SegJob is filled here, never dereferenced */
#include "pl_seg.h"
#include "pl_plan.h"
#include "pl_seg_pace.h"
#include "pl_deal.h"
#include "pl_layout.h"
#include "pl_search.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <functional>
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

#pragma GCC visibility push(hidden)      /* nothing below is part of the library's ABI */

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

#pragma GCC visibility pop               /* (the two types the public header names keep the visibility they have there) */

struct pngloss_hip_ctx {
    /* ---- pl_host.hip: the context's life, the caller's options, the batch pipeline and its record of the last batch ---- */
    int device = 0;
    PlHooks hooks;                   /* (from the environment, at creation) */
    int pin_slot = 0;                /* which pair of CPUs of the affinity set this context's launch thread is pinned into: max(device, contexts created before it in the process) */
    int opt_launch_groups = 0;       /* pngloss_hip_set_option("launch_groups", "2" | "3" | "auto"): see run_seg_engine */
    PlEnginePin opt_engine = PlEnginePin::Auto;   /* pngloss_hip_set_option("engine", ...): Auto = the cost model (or, for tests, $PNGLOSS_HIP_ENGINE) */
    bool opt_distortion = false;     /* pngloss_hip_set_option("distortion", "on" | "off") */
    bool opt_ssim = false;           /* pngloss_hip_set_option("ssim", "on" | "off") */
    /* option "measure": what the two measuring kernels count, behind a batch and in the probes of the target searches: every pixel, or the visible ones
     * (pl_distort_core.h, pl_ssim_core.h).  The pipeline never sees it. */
    bool opt_visible = false;        /* pngloss_hip_set_option("measure", "all" | "visible") */
    bool opt_indexed = false;        /* pngloss_hip_set_option("indexed", "on" | "off") */
    uint32_t opt_index_depth = PLI_DEPTH_8;   /* pngloss_hip_set_option("index_depth", "8" | "auto" | "min"): read where opt_indexed is (pl_index_core.h: PliDepthMode) */
    /* one device arena, regrown on demand, carved per batch */
    GrowBuf d_ws;
    std::vector<PlJob> h_jobs;
    std::vector<uint32_t> h_sel;     /* (stays alive until the asynchronous copy that reads it is done: the next enqueue) */
    size_t n_last = 0;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; /* total start, engine start, engine stop, total stop */
    double engine_ms = -1.0, total_ms = -1.0;
    bool pending = false;
    /* -v progress display of the single-image seam: a host-mapped word the engine writes the finished row count to (BatchCall::want_progress) */
    uint32_t *h_progress = nullptr;
    std::vector<uint8_t> engine;     /* per image of the last batch: the row engine its plan gave it (PLR_ENGINE_*, pl_result.h) */
    const PlDistortRecord *d_records = nullptr;      /* the batch in flight is measured (option "distortion"): its records, copied back by finish */
    std::vector<pngloss_hip_distortion> distortion;  /* per image of the last finished batch; empty when it ran with the option off */
    const PlSsimRecord *d_ssim_records = nullptr;    /* the batch in flight is measured (option "ssim"): its records, copied back by finish */
    std::vector<pngloss_hip_ssim> ssim;              /* per image of the last finished batch; empty when it ran with the option off */

    /* ---- pl_host_seg.hip: the segment-parallel engine.  Its launch loop runs on a helper thread and on streams of the engine's own (the number of
     * row attempts is decided by the data): the caller's stream waits for the "images finished" word instead of for the host ---- */
    uint32_t *h_seg_words = nullptr; /* host-mapped words (images finished, attempt being started, ...: pl_seg_pace.h) the control kernel writes and the launch loop reads */
    hipStream_t seg_gstream[SEG_MAX_GROUPS] = {};   /* one stream per GROUP of a batch's images (run_seg_engine); [0] has been taken as soon as the engine has run once */
    hipEvent_t ev_seg_gdone[SEG_MAX_GROUPS] = {};   /* engine's streams: behind the last attempt the launch thread enqueued */
    int seg_groups = 1;
    bool seg_async_wait = false;     /* the last batch on the segment engine put a wait for the engine on the caller's stream (the asynchronous entry's non-blocking variant) */
    hipEvent_t ev_prep = nullptr;    /* caller's stream: everything the engine reads is in place */
    std::thread seg_worker;
    std::atomic<int> seg_rc{ 0 };
    std::vector<SegJob> h_sj;        /* (stay alive until the asynchronous copies that read them are done: the next enqueue) */
    SegParams h_seg_params;
    int stream_wait_ok = -1;         /* hipStreamWaitValue32 usable on this device (-1: not asked yet) */
    int seg_prio = 0;
    bool seg_prio_distinct = false;

    /* ---- pl_host_window.hip: host-pointer batches (pngloss_hip_optimize_batch_host*): a persistent device arena and a persistent pinned staging
     * buffer of the same layout, both regrown on demand -- no hipMalloc/hipFree and no pageable copies per call ---- */
    GrowBuf d_arena;
    GrowBuf h_pinned{ true };
    hipStream_t copy_stream = nullptr;               /* (ensure_copy_stream) */
    double upload_ms = -1.0, download_ms = -1.0, deflate_ms = -1.0;
    bool split_last = false;         /* the last host window ran in chunks: images behind n_last are the peers' */
    std::vector<pngloss_hip_ctx *> peers;   /* further contexts on the same device: the other chunks of a host window (batch_host) */
    std::vector<size_t> chunk_first; /* first image of every chunk of the last split window (chunk 0 is this context's) */
    /* option "indexed": the index workspace (pl_layout.h: pl_index_layout -- job table, counters, palette records, colour tables, index rows), regrown on
     * demand like the others; used by the deflate stage of a host window (window_index) */
    GrowBuf d_index;
    std::vector<pngloss_hip_palette> palette;        /* per image of the last finished host window that returned zlib streams with the option on; else empty */
    std::vector<pngloss_hip_index_depth> index_depth;   /* ... and beside it which bit depth was kept, from which sizes (option "index_depth"; the packed rows lie behind the index workspace in d_index) */

    /* ---- pl_host_measure.hip: the tables of the two measuring kernels ---- */
    /* options "distortion" and "ssim": the keep arena (pl_layout.h: job table, records, the originals pl_keep copies -- one arena, one pl_keep launch for
     * both options), regrown on demand like the others */
    GrowBuf d_keep;
    std::vector<PlDistortJob> h_dj;  /* (stays alive until the asynchronous copy that reads it is done: the next enqueue) */
    /* the SSIM kernel's job table and records live in a small buffer of their own (pl_layout.h: pl_ssim_layout), regrown on demand like the others */
    GrowBuf d_ssim;
    std::vector<PlSsimJob> h_ssj;    /* (stay alive until the asynchronous copies that read them are done: the next enqueue) */
    std::vector<PlSsimRecord> h_ssr;

    /* ---- pl_host_search.hip: the search arena (pl_target.h: tables, originals, best results so far), regrown on demand like the others ---- */
    GrowBuf d_target;

    /* ---- pl_host_read.hip: device frames of pngloss_hip_png_decode_batch_device: decoded RGBA8 that stays on the device for the optimiser ---- */
    GrowBuf d_frames;

    /* ---- pl_host_quant.hip: the quantiser's workspace (pl_layout.h: pl_quant_layout), regrown on demand like the others ---- */
    GrowBuf d_quant;
};

/* all the GPUs of the node (pl_host_window.hip): one context per device */
struct pngloss_hip_multi {
    std::vector<pngloss_hip_ctx *> ctx;
    std::vector<std::pair<int, size_t>> where;   /* per image of the last call: the context it went to, and its index in that context's batch */
};

#pragma GCC visibility push(hidden)

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
static_assert(PLD_MAX_IMAGES == PLS_MAX_IMAGES && PLD_MAX_IMAGES == 65535, "the measuring launches slice a batch at the same place: gridDim.y holds 65535 images");

struct EmitTarget { void *d_ids; void *d_rows; uint32_t pitch; };

/* What to measure behind a batch: the distortion records, the SSIM records, and whether the two count the visible pixels or all of them
 * (pl_distort_core.h, pl_ssim_core.h).  The pipeline never sees it. */
struct Measure {
    bool distortion = false, ssim = false, visible = false;
    bool indexed = false;       /* option "indexed": not a measurement, but it travels the same way -- the deflate stage of a host window (window_index) reads it, nothing else does */
    uint32_t index_depth = PLI_DEPTH_8;   /* option "index_depth": beside it, read where it is on */
};
/* ... as the caller's options ask for it: what the plain entry points hand on (no context: nothing; the call fails where it always did) */
inline Measure measure_of_options(const pngloss_hip_ctx *c) { return c ? Measure{ c->opt_distortion, c->opt_ssim, c->opt_visible, c->opt_indexed, c->opt_index_depth } : Measure{}; }

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

/* ---- pl_host.hip ---- */
int enqueue(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const BatchCall &call);
int finish(pngloss_hip_ctx *ctx, pngloss_hip_result *results, size_t n);
/* The context has no "last batch" to index (pngloss_hip_last_*): enqueue begins every batch with it (only a split host window sets split_last again: batch_host) */
void forget_last_batch(pngloss_hip_ctx *c);
/* A search runs many batches of its own on the context: whatever happens, no "last batch" to index behind it -- for the host forms (peers), none
 * on the peers the host windows ran their other chunks on either */
struct SearchGuard {
    pngloss_hip_ctx *c; bool peers;
    ~SearchGuard() { forget_last_batch(c); if (peers) for (pngloss_hip_ctx *p : c->peers) if (p) forget_last_batch(p); }
};

/* the width / height vectors of a batch: of pngloss_hip_image_desc or of pngloss_hip_host_image */
template <class Image> void batch_dims(const Image *images, size_t n, std::vector<uint32_t> &width, std::vector<uint32_t> &height)
{
    width = std::vector<uint32_t>(n); height = std::vector<uint32_t>(n);
    for (size_t i = 0; i < n; i++) { width[i] = images[i].width; height[i] = images[i].height; }
}
/* A context takes one batch at a time.  The refusal of a call that would start another one ... */
inline bool previous_batch_refused(const pngloss_hip_ctx *ctx)
{
    if (!ctx->pending) return false;
    std::fprintf(stderr, "pngloss_hip: previous batch not finished; call pngloss_hip_finish first\n");
    return true;
}
/* ... and of one that needs the buffers the batch in flight works in (the comparisons, the read side) */
inline bool batch_in_flight_refused(const pngloss_hip_ctx *ctx)
{
    if (!ctx->pending) return false;
    std::fprintf(stderr, "pngloss_hip: a batch is in flight on this context; call pngloss_hip_finish first\n");
    return true;
}

/* ---- pl_host_seg.hip ---- */
/* process-wide: has any context put a wait for the engine on a caller's stream (written by run_seg_engine, read by enqueue for the plan's launch groups) */
extern std::atomic<bool> g_stream_wait_used;
int run_seg_engine(pngloss_hip_ctx *ctx, const PlJob *d_jobs, const PlPlan &plan, const PlBatchLayout &lay, const BatchCall &call,
                   const uint32_t *d_sel, const PlEngineParams &prm);
/* a context that is destroyed: its engine streams back to the process's list, its events and words freed */
void seg_engine_release(pngloss_hip_ctx *ctx);

/* ---- pl_host_window.hip ---- */
int ensure_copy_stream(pngloss_hip_ctx *ctx);       /* the context's own non-blocking stream for a window's copies and kernels, created on first use */
int batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n, unsigned quantization_strength,
               long bleed_divider, Measure measure, pngloss_hip_result *results, pngloss_hip_scanlines *lines,
               pngloss_hip_zstream *zs = nullptr);
/* A batch of host images over the contexts of the node, the one shape of every pngloss_hip_multi_optimize_batch_host* call: share(context, its images) -> code */
int deal_over_contexts(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, pngloss_hip_result *results,
                       pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams, bool indexes_last,
                       const std::function<int(pngloss_hip_ctx *, HostSubset &)> &share);
/* The deflate stage, as window_deflate, window_index and size_search run it: what the device deflate (pl_deflate.h) answers, as a code of the ABI ... */
int deflate_rc(hipError_t e);
/* ... what it is to look at: `height` scanlines of `rowbytes` bytes, `pitch` apart, and their filter types; out: where the stream goes, or nullptr (a measuring pass) ... */
pl_deflate_image deflate_image_of(const void *d_filter_types, const void *d_scanlines, uint32_t pitch, uint32_t rowbytes, uint32_t height,
                                  unsigned char *out = nullptr, size_t out_capacity = 0);
/* ... the caller's stream record before the stage (no stream, truecolour with alpha, no blocks) and behind it (size and block counts of a finished image) */
void zstream_clear(pngloss_hip_zstream &z);
void zstream_take(pngloss_hip_zstream &z, const pl_deflate_image &d);

/* ---- pl_host_measure.hip ---- */
void fill_distort_jobs(PlDistortJob *jobs, PlDistortRecord *d_records, size_t n, const void *const *img, const void *const *keep, const uint64_t *pixels);
int upload_distort_jobs(pngloss_hip_ctx *ctx, const PlKeepLayout &lay, size_t n, const void *const *img, const void *const *keep, const uint64_t *pixels, hipStream_t stream);
uint64_t fill_ssim_jobs(PlSsimJob *jobs, PlSsimRecord *records, PlSsimRecord *d_records, size_t n, const void *const *a, const void *const *b,
                        const uint32_t *width, const uint32_t *height, bool visible);
int upload_ssim_jobs(pngloss_hip_ctx *ctx, size_t n, const void *const *a, const void *const *b, const uint32_t *width, const uint32_t *height,
                     hipStream_t stream, PlSsimLayout &lay, uint64_t &max_tiles, bool visible);

/* ---- pl_host_quant.hip: the checks and the stages of a quantiser call, which pl_host_quant_target.hip runs too ---- */
int check_quant_params(const pngloss_hip_quant_params2 *params);
/* every image with pixels has a pointer (pixels_of[i]) and few enough pixels (plq_pixels_ok) */
int check_quant_pixels(const uint32_t *width, const uint32_t *height, size_t n, const void *const *pixels_of);
/* the whole workspace of a call: the quantiser's, and behind it -- when the call dithers -- the dither pass's job table and error lines */
struct QuantWorkspace {
    PlQuantLayout lay;
    PlDitherLayout dither;
    bool dithers = false;
    bool visible = false;       /* the call runs in the premultiplied space (include/pngloss_hip_quant_space.h): no byte of the workspace differs, the kernels do */
    size_t total() const { return dithers ? dither.total : lay.total; }
};
QuantWorkspace quant_workspace_of(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool inputs, const pngloss_hip_quant_params2 &params,
                                  uint32_t space);
/* One call's images in the workspace ctx->d_quant, which the caller has grown to ws.total(): what quant_survey finds out about them and the job
 * tables the later stages launch over.  Entry k of ijobs / qjobs is image live[k]; hists holds PLQ_BINS counts per entry, on the host. */
struct QuantBatch {
    pngloss_hip_ctx *ctx;
    const QuantWorkspace &ws;
    const std::vector<uint32_t *> &img;
    const std::vector<uint32_t> &width, &height;
    hipStream_t stream;
    std::vector<size_t> live;                       /* the images with pixels */
    std::vector<PlIndexJob> ijobs;
    std::vector<PlQuantJob> qjobs;
    uint64_t max_pixels = 0;
    std::vector<uint32_t> counts, hists;
    char *base() const { return ctx->d_quant.p; }
    const PlIndexJob *d_ijobs() const { return reinterpret_cast<const PlIndexJob *>(base() + ws.lay.index_jobs); }
    const PlQuantJob *d_qjobs() const { return reinterpret_cast<const PlQuantJob *>(base() + ws.lay.quant_jobs); }
};
int quant_survey(QuantBatch &b, pngloss_hip_quant_report *reports);
int quant_first_palette(QuantBatch &b, size_t k, uint32_t colors, std::vector<uint32_t> &pals);
int quant_refine(QuantBatch &b, const std::vector<size_t> &work, const std::vector<uint32_t> &pals, uint32_t rounds, std::vector<PlQuantJob> &jobs, uint64_t &work_pixels);
int quant_dither(QuantBatch &b, const std::vector<size_t> &work);
int quant_close(QuantBatch &b, const std::vector<PlQuantJob> &jobs, uint64_t work_pixels, const std::vector<size_t> &pass, const std::vector<uint32_t> &allowed,
                pngloss_hip_quant_report *reports);
/* The calls themselves, behind every entry point of theirs: the older ones hand in PNGLOSS_HIP_QUANT_SPACE_RGBA, those of pl_host_quant_space.hip the
 * space of their record, which they have checked (0 or 1); every other check is made here, before any device work */
int quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                   pngloss_hip_quant_report *reports, void *stream);
int multi_quantize_batch_host(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                              pngloss_hip_quant_report *reports);
/* ---- pl_host_quant_target.hip ---- */
int quantize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                          const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream);
int multi_quantize_batch_host_target(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params2 *params, uint32_t space,
                                     const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports);

#pragma GCC visibility pop

#endif

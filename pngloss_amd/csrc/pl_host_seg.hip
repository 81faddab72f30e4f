/*
 * pl_host_seg.hip -- the host side of the segment-parallel engine: the process's pool of engine streams, the launch thread, run_seg_engine
 * (pl_host_ctx.h has the map of the host files).  When a group gets its next attempt and when the loop gives up is pl_seg_pace.h's to say; how a
 * batch is cut into groups is pl_plan.h's.
 */
#include "pl_host_ctx.h"

#include <pthread.h>
#include <sched.h>

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
std::atomic<bool> g_stream_wait_used{ false };
static std::atomic<bool> g_third_engine_stream{ false };

namespace {
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
    ctx->seg_rc.store(rc, std::memory_order_release);
}
} // namespace

int run_seg_engine(pngloss_hip_ctx *ctx, const PlJob *d_jobs, const PlPlan &plan, const PlBatchLayout &lay, const BatchCall &call,
                   const uint32_t *d_sel, const PlEngineParams &prm)
{
    const hipStream_t stream = call.stream;
    const std::vector<uint32_t> &list = plan.seg_list;
    const size_t n = list.size();                              /* the images of the batch this engine takes */
    const int ngroups = plan.ngroups;                          /* (launch groups: pl_plan_batch) */
    if (!ctx->h_seg_words) PL_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_seg_words), sizeof(uint32_t) * PL_SEG_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    if (!ctx->seg_gstream[0]) {
        /* a stream of the HIGHEST priority: streams of one priority share a few hardware queues, and a queue whose head is a caller's
         * wait for the finished word holds up everything behind it -- the engine's attempts must never sit in such a queue (twelve
         * contexts with twelve waiting streams deadlocked that way before this stream had a priority of its own) */
        int least = 0, greatest = 0;
        PL_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        ctx->seg_prio = greatest;
        PL_CHECK(seg_stream_pool().take(ctx->device, greatest, &ctx->seg_gstream[0]));
        ctx->seg_prio_distinct = greatest != least;
    }
    if (!ctx->ev_prep) PL_CHECK(hipEventCreateWithFlags(&ctx->ev_prep, hipEventDisableTiming));
    if (!ctx->ev_seg_gdone[0]) PL_CHECK(hipEventCreateWithFlags(&ctx->ev_seg_gdone[0], hipEventDisableTiming));
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

void seg_engine_release(pngloss_hip_ctx *ctx)
{
    for (int g = SEG_MAX_GROUPS - 1; g >= 0; g--) if (ctx->seg_gstream[g]) { (void)hipStreamSynchronize(ctx->seg_gstream[g]); seg_stream_pool().give(ctx->device, ctx->seg_gstream[g]); }   /* (back to the process's list, [0] first) */
    for (int g = 0; g < SEG_MAX_GROUPS; g++) if (ctx->ev_seg_gdone[g]) (void)hipEventDestroy(ctx->ev_seg_gdone[g]);
    if (ctx->ev_prep) (void)hipEventDestroy(ctx->ev_prep);
    if (ctx->h_seg_words) (void)hipHostFree(ctx->h_seg_words);
}

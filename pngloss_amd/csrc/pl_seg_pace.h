/*
 * pl_seg_pace.h -- the decisions of the segment engine's launch loop, as pure functions of plain inputs: the host-visible words the loop shares with the
 * device, when a launch group gets its next row attempt (look-ahead throttle, runaway bound, the switch away from seeds), what the loop does when it has
 * nothing to launch (stall watchdog, back-off), what it reports, which CPU the launch thread takes and whether the caller's stream waits on the device.
 * Internal.
 *
 * Plain C++17 without HIP: pl_host_seg.hip (seg_worker_main, run_seg_engine) makes the calls -- launches, events, yield and sleep -- and asks here what to do;
 * tests/c/pace_host.cpp compiles the same header with g++ and drives it with a scripted device (tests/test_pace_host.py).  Everything is inline and fixed
 * in size: the thread issues four launches every 45 - 100 us.  Nothing here changes results: every pace gives the reference's bytes.
 */
#ifndef PL_SEG_PACE_H
#define PL_SEG_PACE_H

#include "pl_plan.h"

#include <cstddef>
#include <cstdint>

/* ---- the host-visible words: per launch group g the images of the group that are finished (SegJob::done_counter, every image adds itself), the attempt
 * its first image is working on (SegJob::attempt_word) and the rows the chain kernel broke off (SegJob::break_word) ---------------------------------------- */
constexpr int PL_SEG_WORDS = 4 * SEG_MAX_GROUPS;     /* (three are used per group) */
constexpr int pl_seg_done_word(int g) { return 2 * g; }
constexpr int pl_seg_attempt_word(int g) { return 2 * g + 1; }
constexpr int pl_seg_break_word(int g) { return 2 * SEG_MAX_GROUPS + g; }
struct PlSegWords { uint32_t done, attempt, breaks; };       /* one reading of a group's three */
inline PlSegWords pl_seg_words_read(const volatile uint32_t *words, int g)
{
    PlSegWords w;
    w.done = words[pl_seg_done_word(g)];
    w.attempt = words[pl_seg_attempt_word(g)];
    w.breaks = words[pl_seg_break_word(g)];
    return w;
}

/* ---- the pace of the launches ------------------------------------------------------------------------------------------------------------------------------ */
constexpr long PL_SEG_LOOKAHEAD = 32;                  /* attempts queued ahead of the one the device works on */
constexpr int64_t PL_SEG_STALL_NS = 20000000000ll;     /* no attempt word has moved for longer than this: the engine has stopped */

struct PlSegPace {
    struct Group {
        uint32_t n;          /* images */
        bool seeds;          /* SegShape::seeds of the group's next attempt: once off, off for the rest of the batch */
        long launched;
        uint32_t seen;       /* the attempt word at the last poll */
    } g[SEG_MAX_GROUPS];
    int ngroups;
    long max_attempts;       /* pl_seg_max_attempts */
    int64_t t_last;          /* when an attempt word last moved */
    int idle;                /* polls without a launch since then */
    long lead_sum, lead_n, lead_min, lead_low;   /* (PNGLOSS_HIP_DEBUG) how far ahead of the device the launches run, from a group's 65th on: sum, count, least, at most two ahead */
};
/* now: any steady clock, in nanoseconds.  Then every group's images and the SegShape::seeds its attempts begin with */
inline PlSegPace pl_seg_pace_begin(int ngroups, long max_attempts, int64_t now)
{
    PlSegPace p{};
    p.ngroups = ngroups;
    p.max_attempts = max_attempts;
    p.t_last = now;
    p.lead_min = 1 << 30;
    return p;
}

inline void pl_seg_pace_group(PlSegPace &p, int g, size_t n, bool seeds) { p.g[g].n = (uint32_t)n; p.g[g].seeds = seeds; }

enum class PlSegStep { Finished, Busy, Runaway, Launch };
/* One poll of group g.  Finished: its images are through.  Busy: the device has its look-ahead queued.  Runaway: more attempts than any image can need.
 * Launch: attempt number g[g].launched, with g[g].seeds; pl_seg_pace_launched() once it is enqueued.
 * An attempt word that moved is progress: it restarts the stall clock and the back-off. */
inline PlSegStep pl_seg_pace_poll(PlSegPace &p, int g, const PlSegWords &w, int64_t now)
{
    PlSegPace::Group &G = p.g[g];
    if (w.done >= G.n) return PlSegStep::Finished;
    if (w.attempt != G.seen) { G.seen = w.attempt; p.t_last = now; p.idle = 0; }
    const long lead = G.launched - (long)w.attempt;
    if (lead > PL_SEG_LOOKAHEAD) return PlSegStep::Busy;
    if (G.launched > p.max_attempts) return PlSegStep::Runaway;
    /* a group whose rows keep breaking off -- its images hold fixed points and cycles the seeds do not reach (flat content; real photographs break in ~5 % of their rows,
     * the generator's frames in 0.3 %) -- goes back to the start from every state for the rest of the batch: more than one image-row in 25, sixteen to begin with (the
     * device-side rule, seg_unit_from_seeds, does the same image by image inside the kernel; this one changes the KERNEL -- for small batches seg_k_enum instead of
     * seg_k_enum_unit<1> with its slow exhaustive path).  Results do not depend on it; the count lags the launches by the look-ahead. */
    if (G.seeds && (uint64_t)w.breaks * 25u > (uint64_t)w.attempt * G.n + 400u) G.seeds = false;
    if (G.launched >= 64) { p.lead_sum += lead; p.lead_n++; if (lead < p.lead_min) p.lead_min = lead; if (lead <= 2) p.lead_low++; }
    return PlSegStep::Launch;
}
inline void pl_seg_pace_launched(PlSegPace &p, int g) { p.g[g].launched++; }

enum class PlSegIdle { Stalled, Yield, Sleep };
/* after a poll of every group in which nothing was launched: every group has its look-ahead queued -- leave the core to others, the first three times by
 * yielding, then by sleeping 100 us (a row attempt takes 50 - 200 us) */
inline PlSegIdle pl_seg_pace_idle(PlSegPace &p, int64_t now)
{
    if (now - p.t_last > PL_SEG_STALL_NS) return PlSegIdle::Stalled;
    return ++p.idle < 4 ? PlSegIdle::Yield : PlSegIdle::Sleep;
}

/* pngloss_hip_last_seg_attempts: the attempts of the group that took the most */
inline long pl_seg_pace_attempts(const PlSegPace &p)
{
    long mx = 0;
    for (int g = 0; g < p.ngroups; g++) mx = p.g[g].launched > mx ? p.g[g].launched : mx;
    return mx;
}
/* whatever went wrong, the caller's stream must not wait for ever: the finished word of every group g says that all of its n images are through (they are NOT:
 * the error is reported by pngloss_hip_finish) */
inline void pl_seg_words_release(volatile uint32_t *words, int g, size_t n) { words[pl_seg_done_word(g)] = (uint32_t)n; }

/* ---- the CPU of the launch thread --------------------------------------------------------------------------------------------------------------------------
 * CPU (2 * slot + 1) of the process's affinity set (cpus[0 .. ncpus), ascending), slot = the context's device ordinal or its serial number in the process,
 * whichever is larger: eight ranks with one device each and eight contexts of one process get eight different CPUs.  -1, the thread stays where the scheduler
 * puts it: the set is too small for that, or pin_hook (PNGLOSS_HIP_PIN) is 0. */
inline int pl_seg_pin_cpu(const int *cpus, size_t ncpus, int pin_slot, int pin_hook)
{
    const size_t want = (size_t)(2 * pin_slot + 1);
    return pin_hook != 0 && ncpus >= 4 && want < ncpus ? cpus[want] : -1;
}

/* ---- does the caller's stream wait for the finished words ON THE DEVICE (hipStreamWaitValue32), or the call for the launch loop on the host ---------------------
 * On the device when the stream memory operation is usable, the engine's streams have a priority of their own (a waiting stream of the engine's priority could
 * share a hardware queue with its attempts), the entry point is not a synchronous one (its caller waits on the host anyway), the process has no third engine
 * stream (pl_plan_batch: launch groups) and the caller's stream -- the default stream apart -- is known to have another priority than the engine's. */
inline bool pl_seg_wait_on_device(bool stream_wait_ok, bool prio_distinct, bool sync_call, bool third_engine_stream, bool default_stream, bool caller_prio_known, int caller_prio, int seg_prio)
{
    if (!stream_wait_ok || !prio_distinct || sync_call || third_engine_stream) return false;
    return default_stream || (caller_prio_known && caller_prio != seg_prio);
}

#endif

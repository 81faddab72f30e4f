/*
 * pl_plan.h -- every decision the library makes about a batch, as pure functions of plain inputs: the pin of the row engine, which row engine
 * takes which image (the cost model), the segment engine's per-image workspace (one table of its arrays: their sizes, offsets and the pointers of a
 * job record), its launch groups and enumeration kind, the runaway bound of its launch loop (pl_seg_max_attempts; the loop's other rules: pl_seg_pace.h),
 * and the chunks of a host window.  Internal.
 *
 * Plain C++17 without HIP: pl_host.hip carries the plan out (workspace, job tables, streams, launches), and tests/c/plan_host.cpp compiles the
 * same header with g++ so that the CPU suite pins the decisions (tests/test_plan_host.py); tests/c/seg_host.cpp binds the workspace of the kernel bodies it
 * runs through the same table.  Nothing here changes results: every engine, group and enumeration kind gives the reference's bytes; the plan decides how fast.
 */
#ifndef PL_PLAN_H
#define PL_PLAN_H

#include "pl_seg_launch.h"

#include <algorithm>
#include <cstring>
#include <vector>

#define SEG_MAX_GROUPS 8

/* ---- the pin of the row engine: pngloss_hip_set_option(ctx, "engine", ..), else $PNGLOSS_HIP_ENGINE (the tests' hook, read once per call) ---- */
enum class PlEnginePin { Auto, Seg, Wg, Lead, Legacy, Mix, Rows };
/* "wg" / "lead" / "legacy" / "mix": the one-workgroup-per-image engine -- "lead": never fall back adaptively, "legacy": round-1 chains only, "mix": alternate every
 * four rows.  "rows": the library's choice, strength 0 included (a no-op at other strengths).  "auto": the library's choice. */
static const struct { const char *name; PlEnginePin pin; } PL_ENGINE_PINS[] = {
    { "auto", PlEnginePin::Auto }, { "seg", PlEnginePin::Seg }, { "wg", PlEnginePin::Wg }, { "lead", PlEnginePin::Lead },
    { "legacy", PlEnginePin::Legacy }, { "mix", PlEnginePin::Mix }, { "rows", PlEnginePin::Rows },
};
/* false for a name that is not in the table */
inline bool pl_engine_pin_parse(const char *s, PlEnginePin *out)
{
    for (const auto &p : PL_ENGINE_PINS)
        if (std::strcmp(s, p.name) == 0) { *out = p.pin; return true; }
    return false;
}
/* the environment's pin: unset or empty is the library's choice, a name the table does not know the one-workgroup-per-image engine */
inline PlEnginePin pl_engine_pin_of_env(const char *s)
{
    PlEnginePin p = PlEnginePin::Auto;
    if (s && *s && !pl_engine_pin_parse(s, &p)) p = PlEnginePin::Wg;
    return p;
}

/* Timing / test hooks of the environment, read ONCE, when a context is created (pngloss_hip_create) -- not per call.  None of them changes results: they pin choices the library
 * otherwise makes itself (launch groups, units, workgroup sizes), pick the blocking variant of the asynchronous entry, or print.  The one hook that is read per call is
 * PNGLOSS_HIP_ENGINE (the tests' pin of the row engine, read once at the top of enqueue; pngloss_hip_set_option(ctx, "engine", ..) takes precedence).  A hook that DOES change results
 * -- "candidate f wins every row", a debugging aid of rounds 1-3 -- exists in builds made with -DPL_DEBUG_FORCE_FILTER=f only: no environment variable of the shipped library can
 * make the drop-in seam write anything but the reference's bytes. */
struct PlHooks {
    int seg_groups = 0;          /* PNGLOSS_HIP_SEG_GROUPS: launch groups of a batch on the segment engine (0: the library's choice) */
    bool no_stream_wait = false; /* PNGLOSS_HIP_NO_STREAM_WAIT: the blocking variant of the asynchronous entry (rocprofv3 --pmc needs it) */
    int seg_unit = -1;           /* PNGLOSS_HIP_SEG_UNIT: 0 / 1 pins the enumeration per segment / in units (-1: the library's choice) */
    int tparts = 0;              /* PNGLOSS_HIP_SEG_TPARTS */
    int enum_nt = 0;             /* PNGLOSS_HIP_ENUM_NT: 512 / 1024 */
    int kin = -1;                /* PNGLOSS_HIP_KIN: run-in pixels of the seeded enumeration */
    int seg_seeds = -1;          /* PNGLOSS_HIP_SEG_SEEDS: 0 = units start from every state, as in round 5 (-1 / 1: from seeds where the pair has a seed set) */
    int seg_seeds1 = -1;         /* PNGLOSS_HIP_SEG_SEEDS1: 0 / 1 pins the per-segment enumeration from seeds (seg_k_enum_unit<1>; -1: batches of two or more images) */
    int pin = -1;                /* PNGLOSS_HIP_PIN: 0 = the launch thread is not pinned to a CPU (-1 / 1: pinned when the affinity set has room, pl_seg_pace.h:pl_seg_pin_cpu) */
    int calib = -1;              /* PNGLOSS_HIP_CALIB: 1 = the cost model that picks the row engine of a batch is calibrated on this device by a probe (engine_calib; off by default: see enqueue) */
    int seed_kin = -1;           /* PNGLOSS_HIP_SEED_KIN: run-in pixels of the units' seeds (1 .. SEG_SEED_KMAX) */
    bool segprof = false;        /* PNGLOSS_HIP_SEGPROF: phase clocks inside the kernels (slows them down) */
    bool debug = false;          /* PNGLOSS_HIP_DEBUG */
    bool debug_seam = false;     /* PNGLOSS_HIP_DEBUG_SEAM */
    bool force_careful = false;  /* PNGLOSS_HIP_FORCE_CAREFUL: the int16-wrap variant of the round-1 chains for every row (same bytes) */
    bool no_split = false;       /* PNGLOSS_HIP_NO_SPLIT */
    int split = 0;               /* PNGLOSS_HIP_SPLIT: chunks of a host window */
};

/* ---- the segment engine's per-image workspace, stated ONCE: one 256-B aligned carve per image, its arrays in this order --------------------------------------
 * X(field of SegJob, elements): the element type is the field's own (pl_seg_core.h says what each array holds); the counts may use width, nseg, ngrp, nsp and
 * seeded.  pl_seg_layout() turns the table into offsets and exact byte sizes, pl_seg_bind() into the pointers of a SegJob -- for the library at base + offset
 * (run_seg_engine), for the CPU harness a heap block of exactly the array's bytes each (tests/c/seg_host.cpp: the sanitizers check the product's sizes). */
#define PL_SEG_ARRAYS(X)                                                                       \
    X(ctl, 3)                                                                                  \
    X(base, 3 * SEG_NFILT * 256)                                                               \
    X(H0, 3 * 256)                                                                             \
    X(acc, 3)                                                                                  \
    X(err0, (size_t)width * 4)                                                                 \
    X(err1, (size_t)width * 4)                                                                 \
    X(rowcopy, (size_t)width * 3)                                                              \
    X(tables, (size_t)SEG_NFILT * SEG_TBL_WORDS)                                               \
    X(maps, seeded ? 0 : (size_t)SEG_NFILT * nseg * 4 * nsp)                                   \
    X(ehash, seeded ? (size_t)SEG_NFILT * nseg * 4 * SEG_EH_WORDS : 0)                         \
    X(rout, (size_t)SEG_NFILT * nseg * 4 * SEG_NSP)                                            \
    X(rst, (size_t)SEG_NFILT * nseg * 4 * SEG_NSP)                                             \
    X(rck, (size_t)SEG_NFILT * nseg * 4 * SEG_NSP * (SEG_PARTS - 1))                           \
    X(dnout, (size_t)SEG_NFILT * nseg * 4)                                                     \
    X(dcnt, (size_t)SEG_NFILT * nseg * 4)                                                      \
    X(entry, (size_t)SEG_NFILT * nseg * 4)                                                     \
    X(segcnt, (size_t)SEG_NFILT * nseg * 256)                                                  \
    X(grpcnt, (size_t)SEG_NFILT * ngrp * 256)                                                  \
    X(grpleft, (size_t)SEG_NFILT * ngrp)                                                       \
    X(firstidx, SEG_NFILT * 4 * 2)                                                             \
    X(rowmm, 2 * 2)
struct PlSegArray { size_t off, bytes; };       /* bytes: what the array holds, exactly; the carve gives an empty one 4 bytes and rounds every one up to 256 */
struct PlSegLayout {
#define PL_SEG_X(name, count) PlSegArray name;
    PL_SEG_ARRAYS(PL_SEG_X)
#undef PL_SEG_X
    size_t total; uint32_t nseg, ngrp;
};
/* width: the image's, 1 for an image without pixels (w ? w : 1); nsp, seeded: SegParams::nsp / ::seeded of the (strength, bleed) pair */
inline PlSegLayout pl_seg_layout(uint32_t width, uint32_t nsp, bool seeded)
{
    PlSegLayout l{};
    const uint32_t nseg = l.nseg = (width + SEG_L - 1) / SEG_L;
    const uint32_t ngrp = l.ngrp = (nseg + SEG_GRP - 1) / SEG_GRP;
    size_t o = 0;
    auto take = [&](size_t bytes) { const PlSegArray a{ o, bytes }; o = (o + (bytes ? bytes : 4) + 255) / 256 * 256; return a; };
#define PL_SEG_X(name, count) l.name = take(sizeof(*SegJob::name) * (size_t)(count));
    PL_SEG_ARRAYS(PL_SEG_X)
#undef PL_SEG_X
    l.total = o;
    return l;
}
/* ctl .. rowmm, nseg and ngrp of a SegJob whose image is `width` pixels wide (0: no segments): storage(a) is where array a lives */
template <class Storage>
inline void pl_seg_bind(SegJob &j, const PlSegLayout &l, uint32_t width, Storage &&storage)
{
#define PL_SEG_X(name, count) j.name = (decltype(j.name))storage(l.name);
    PL_SEG_ARRAYS(PL_SEG_X)
#undef PL_SEG_X
    j.nseg = width ? l.nseg : 0; j.ngrp = width ? l.ngrp : 0;
}

/* ---- how the segment engine enumerates a row's segments ------------------------------------------------------------------------------------------------------
 * Per segment (one image: the shortest dependent path) or in UNITS of SEG_UNIT segments (seg_enum_unit_body: less than half the instructions per row, a dependent
 * path SEG_UNIT times as long -- it pays when the batch is what keeps the GPU busy, not the latency of one row: from a handful of images on); each from every state
 * or -- round 6, where the (strength, bleed) pair has a seed set -- from seeds with a run-in.  State sets beyond the lanes are always SEEDED (seg_k_enum_seeded).
 * Results do not depend on it: the validation is the ground truth either way. */
enum class PlEnumKind { SegAll, SegSeeds, UnitsAll, UnitsSeeds, Seeded };
/* segs, k: segments and images of the segment engine's share of the batch.  The pins (-1: the library's choice) are the hooks PNGLOSS_HIP_SEG_UNIT, _SEG_SEEDS and
 * _SEG_SEEDS1; the cost model passes seg_seeds only. */
inline PlEnumKind pl_enum_kind(size_t segs, size_t k, const SegParams &P, int seg_unit = -1, int seg_seeds = -1, int seg_seeds1 = -1)
{
    if (P.seeded) return PlEnumKind::Seeded;
    const bool can = P.ns <= SEG_NSP;       /* (state sets of one chunk of lanes: with more, the distinct states of a workgroup's pairs outgrow its lanes) */
    const bool have_seeds = can && P.seed_n > 0 && seg_seeds != 0;
    /* (with seeds the per-segment enumeration stays ahead up to sixteen 1080p frames: pl_seg_core.h -- where it applies: batches of NARROW images, which it does not take, go to units from
     *  the round-5 size on: 40 photographs of 512 .. 768 pixels, 784 segments, 54.8 ms in units against 62.4 per segment from every state) */
    const bool seeds1_fit = have_seeds && k >= 2 && segs >= SEG_SEEDS1_MIN_SEGS && segs >= (size_t)SEG_SEEDS1_MIN_SEGS_PER_IMAGE * k;
    bool units = can && segs > (seeds1_fit ? (size_t)SEG_UNIT_MIN_SEGS_SEEDS : (size_t)SEG_UNIT_MIN_SEGS);
    if (seg_unit >= 0) units = can && seg_unit != 0;
    if (units) return have_seeds ? PlEnumKind::UnitsSeeds : PlEnumKind::UnitsAll;
    /* a batch of two or more images below the units' size goes segment by segment from seeds, through the same bodies (seg_k_enum_unit<1>) */
    if (have_seeds && (seg_seeds1 >= 0 ? seg_seeds1 != 0 : seeds1_fit)) return PlEnumKind::SegSeeds;
    return PlEnumKind::SegAll;
}
inline bool pl_enum_in_units(PlEnumKind k) { return k == PlEnumKind::UnitsAll || k == PlEnumKind::UnitsSeeds; }
inline bool pl_enum_from_seeds(PlEnumKind k) { return k == PlEnumKind::UnitsSeeds || k == PlEnumKind::SegSeeds; }

/* ---- the plan of a batch ---------------------------------------------------------------------------------------------------------------------------------------- */
struct PlPlanInput {
    std::vector<uint32_t> width, height;    /* per image (zeros allowed) */
    unsigned strength = 0;
    long bleed = 1;
    PlEnginePin pin = PlEnginePin::Auto;
    PlHooks hooks;
    int forced_filter = -1;                 /* a -DPL_DEBUG_FORCE_FILTER=f build: f (candidate f wins every row -- not the reference's bytes); -1: the shipped library */
    bool rows_fit = true;                   /* the row-statistics engine's counters fit beside the images (the caller's memory check: pl_rows_wanted) */
    double cus = 256.0, seg_scale = 1.0, wg_scale = 1.0;   /* the device's CUs and the cost model's calibration scales (engine_calib) */
    bool sync_call = false, three_groups_ok = false;        /* the context's entry point (pngloss_hip_ctx) */
    int opt_launch_groups = 0;              /* pngloss_hip_set_option("launch_groups", ..) */
    bool stream_wait_used = false;          /* a context of the process has put a wait for the engine on a caller's stream (g_stream_wait_used) */
};
struct PlSegGroupPlan : SegShape {          /* one launch group of the segment engine (PlSegBatch): the shape of its attempts (pl_seg_launch.h) and the number of its images */
    size_t n;
};
struct PlPlan {
    bool use_rows = false;                  /* strength 0: the row-statistics engine takes every image */
    bool seg_costed = false;                /* the cost model chose (the engine was the library's to choose and the segment engine could take the batch) */
    bool seg_pin_unmet = false;             /* "seg" pinned, but no image of the batch fits the segment engine */
    int engine_mode = 0;                    /* PlEngineParams::engine_mode */
    SegParams params = {};                  /* the segment engine's, when seg_list is not empty */
    std::vector<uint8_t> on_seg;
    std::vector<uint32_t> seg_list, wg_list;   /* the segment engine's images tallest first (stable), the others in order */
    PlEnumKind kind = PlEnumKind::SegAll;
    int ngroups = 0;
    size_t gfirst[SEG_MAX_GROUPS + 1] = {}; /* group g = seg_list[gfirst[g] .. gfirst[g + 1]) */
    PlSegGroupPlan group[SEG_MAX_GROUPS] = {};
    long max_attempts = 0;
};

/* The runaway bound of the segment engine's launch loop (pl_seg_pace.h), for images of up to max_h rows: every row needs one attempt per strength it is tried at
 * (pngloss_image.c:266-274: down to 0 in the worst case), every epoch two more (the attempt under way when its validation fails is void): a bound far above
 * anything real, there to stop a runaway loop -- the stall detector of the launch thread is the other net.  (Seen: 1813 attempts for a 63 x 2 image at strength
 * 200, all rows adaptive.) */
inline long pl_seg_max_attempts(uint32_t max_h, int strength)
{
    return (long)std::min<double>(2.0e9, (double)max_h * ((double)strength + 1.0) * (2.0 + 2.0 * SEG_MAX_RESTARTS * SEG_NFILT) + 1024.0);
}

/* STRENGTH 0 has a row engine of its own (pl_rows.hip: nothing is quantised, the five candidate rows are the original row, what is left is the filter search): every
 * image of the batch, unless a test pins another engine -- and unless its counters do not fit (rows_fit).  "rows" pins it (a no-op at other strengths). */
inline bool pl_rows_wanted(unsigned strength, PlEnginePin pin, const PlHooks &hk, int forced_filter)
{
    const bool free_choice = pin == PlEnginePin::Auto || pin == PlEnginePin::Rows;
    return strength == 0 && free_choice && forced_filter < 0 && !hk.force_careful;
}

inline PlPlan pl_plan_batch(const PlPlanInput &in)
{
    PlPlan p;
    const size_t n = in.width.size();
    const PlHooks &hk = in.hooks;
    const auto &W = in.width, &H = in.height;
    p.use_rows = pl_rows_wanted(in.strength, in.pin, hk, in.forced_filter) && in.rows_fit;
    p.engine_mode = in.pin == PlEnginePin::Legacy ? 1 : (in.pin == PlEnginePin::Lead ? 2 : (in.pin == PlEnginePin::Mix ? 3 : 0));
    if (in.forced_filter >= 0) p.engine_mode |= (in.forced_filter + 1) << 8;
    p.on_seg.assign(n, 0);
    /* Which row engine, IMAGE BY IMAGE: one workgroup for the image (pl_engine: batches, narrow images) or the image spread over the
     * whole GPU (pl_seg: few wide images).  The segment engine takes every strength / bleed pair and rows up to SEG_MAX_WIDTH pixels;
     * it pays off while the batch leaves it the machine (its work per row is ~250x redundant by design).  In a mixed batch the two
     * engines run side by side -- the segment engine's images in one launch sequence (blockIdx.y = image) on the engine's own stream,
     * the others as one workgroup each on the caller's.
     * Cost model (measured on 1 .. 64 frames of 512x512 and 1920x1080, tests/tools/gpu_seg_batch.py): a row
     * attempt of the segment engine takes ~38 us plus ~0.032 us per workgroup of its widest kernel (about 3 per segment and 40 more per
     * image), whatever the width, and there are as many attempts as the tallest of its images has rows; the workgroup engine ~0.18 us
     * per pixel of its largest image, all images side by side (256 CUs).  State sets beyond the lanes (s = 85 at bleed 1 or 2 ...) are
     * enumerated from seeds with a run-in of one segment: about twice the enumeration and a wider chain.  Greedy: the images go to the
     * segment engine in the order of their cost on the other one, as long as that shortens the batch. */
    const bool forced = in.pin == PlEnginePin::Seg;
    const bool allowed = in.pin == PlEnginePin::Auto || forced || in.pin == PlEnginePin::Rows;
    SegParams &sp = p.params;
    const bool seg_ok = n && allowed && !p.use_rows && !hk.force_careful && in.strength <= 255 && in.bleed >= 1 && in.bleed <= 32767 &&
                        seg_build_params(sp, (int)in.strength, (int)in.bleed);
    size_t n_seg = 0;
    if (seg_ok) {
        p.seg_costed = !forced;
        const double cu_scale = 256.0 / in.cus;
        /* the cost of one row attempt on the reference box, by enumeration kind: wgs workgroups of the widest kernel, segs segments, k images */
        auto attempt_us_ref = [&](double wgs, double segs, size_t k) {
            switch (pl_enum_kind((size_t)segs, k, sp, -1, hk.seg_seeds)) {
            /* round 6, from seeds (per row of the tallest image, epochs included; 1080p frames, profiles/r06_seeds.txt): units 24 / 32 / 64 / 128 frames 105 / 114 / 168 / 301 us,
             * segment by segment 6 / 11 / 16 frames 61 / 76 / 90 us -- 128 frames 325 ms against 373 on the other engine, the crossover near 148 */
            case PlEnumKind::UnitsSeeds: return std::max(100.0, 35.0 + 0.00945 * wgs);
            case PlEnumKind::SegSeeds: return 43.0 + 0.0134 * wgs;
            /* round 5: a batch whose images have more than SEG_UNIT_MIN_SEGS segments between them is enumerated in UNITS, in two launch groups, with the
             * small workgroups of batches (run_seg_engine): an attempt then takes ~45 us + 0.015 us per workgroup-unit, but not less than ~95 us (the
             * dependent steps of a unit): 1080p frames 16 / 32 / 64 = 102 / 150 / 261 us measured (profiles/r05_unit_groups.txt) */
            case PlEnumKind::UnitsAll: return std::max(100.0, 28.0 + 0.0124 * wgs);   /* (three launch groups, validation in whole replay groups: 16 / 64 / 96 / 112 / 128 frames of 1080p 102 / 205 / 289 / 333 / 377 us: the segment engine up to 116 such frames -- measured: 112 frames 361 against 372 ms, 120 frames 385 against 372) */
            /* (two or more images run as two launch sequences side by side: 4 / 8 / 12 frames of 1080p 58 / 80 / 102 us per attempt, profiles/r05_suite_groups.txt) */
            case PlEnumKind::SegAll: return k >= 2 ? 35.0 + 0.026 * wgs : 38.0 + 0.032 * wgs;
            case PlEnumKind::Seeded: break;
            }
            return 82.0 + 0.05 * wgs;           /* (round 4: an attempt is four launches: 49.5 us at 4096 pixels = 424 workgroups in these units, 46 at 1920, 69 at 8192) */
        };
        auto attempt_us = [&](double wgs, double segs, size_t k) { return in.seg_scale * attempt_us_ref(wgs * cu_scale, segs, k); };      /* (fewer CUs: every workgroup weighs more) */
        auto wg_cost = [&](size_t i) { return in.wg_scale * 0.18 * (double)W[i] * (double)H[i]; };
        std::vector<size_t> order;
        for (size_t i = 0; i < n; i++)
            if (W[i] && H[i] && W[i] <= SEG_MAX_WIDTH) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return wg_cost(x) > wg_cost(y); });
        if (forced) { for (size_t i : order) p.on_seg[i] = 1; n_seg = order.size(); }
        else {
            /* wg side: the largest image left sets its time (or the sum over 256 CUs when there are more images than CUs) */
            double wg_sum = 0;
            for (size_t i = 0; i < n; i++) wg_sum += wg_cost(i);
            double seg_rows = 0, seg_wgs = 0, seg_segs = 0;
            auto batch_us = [&](size_t k, double rows, double wgs, double wsum, double segs) {   /* the first k images of `order` on the segment engine */
                const double wg_us = k < order.size() ? std::max(wg_cost(order[k]), wsum / in.cus) : wsum / in.cus;
                const double seg_us = k ? rows * attempt_us(wgs, segs, k) : 0.0;
                /* side by side only while the other engine leaves the segment engine CUs to run on: its workgroups are persistent and own a CU each (104 KB of
                 * LDS, every register) -- next to 200 and more of them the segment engine's launches wait until they are through: one after the other
                 * (measured: 512 frames of 1080p in one call, 130 of them sent to the segment engine by the model of before: 1034 ms against 2 x 375) */
                if ((double)(n - k) > 0.75 * in.cus) return wg_us + seg_us;
                return std::max(wg_us, seg_us);
            };
            double best = batch_us(0, 0, 0, wg_sum, 0);
            size_t best_k = 0;
            double wsum = wg_sum;
            for (size_t k = 1; k <= order.size(); k++) {
                const size_t i = order[k - 1];
                seg_rows = std::max(seg_rows, (double)H[i]);
                seg_wgs += 3.0 * ((W[i] + SEG_L - 1) / SEG_L) + 40.0;
                seg_segs += (W[i] + SEG_L - 1) / SEG_L;
                wsum -= wg_cost(i);
                if (seg_segs > 8192) break;
                const double t = batch_us(k, seg_rows, seg_wgs, wsum, seg_segs);
                if (t < best) { best = t; best_k = k; }
            }
            for (size_t k = 0; k < best_k; k++) p.on_seg[order[k]] = 1;
            n_seg = best_k;
        }
    }
    p.seg_pin_unmet = forced && !n_seg && n;
    for (size_t i = 0; i < n; i++) (p.on_seg[i] ? p.seg_list : p.wg_list).push_back((uint32_t)i);
    /* the segment engine's images, tallest first: its launch groups are runs of this list, and the tallest image gets a sequence of its own when it stands out */
    std::stable_sort(p.seg_list.begin(), p.seg_list.end(), [&](uint32_t x, uint32_t y) { return H[x] > H[y]; });
    if (!n_seg) return p;

    const std::vector<uint32_t> &list = p.seg_list;
    size_t segs = 0;
    for (size_t i = 0; i < n_seg; i++) segs += (W[list[i]] + SEG_L - 1) / SEG_L;
    /* GROUPS: a batch's images in up to SEG_MAX_GROUPS launch sequences on as many streams.  An attempt is four dependent launches with a latency floor
     * each (the enumeration's dependent steps above all: 75 us with units); images of ONE sequence sit through every floor together, images of different
     * sequences fill each other's floors.  One launch thread feeds all of them. */
    /* (measured, profiles/r05_unit_groups.txt: two sequences 1.2x one from 16 frames of 1080p on, three another 2-6 %, FOUR collapse -- 250 ms for 8 frames
     *  against 113: with the caller's stream they outnumber the hardware queues a process gets, and the stream that shares a queue with the caller's sits
     *  behind its wait for the finished word (without that wait four run, six collapse: profiles/r05_validation_in_enum.txt).  THREE looked 6 % faster in a
     *  process that does nothing else -- and halved every later engine run of bench.py's process, single images included (suite batch 45 -> 14 Mpx/s, 8192 x 8192
     *  137 -> 71): the hardware queues a third engine stream brings into the process's pool stay there, and from then on an engine stream shares one with a
     *  waiting stream.  Two it is for the asynchronous entry: a caller with streams of its own must still fit.  The SYNCHRONOUS entry point puts no wait on
     *  any stream (run_seg_engine): there three groups are safe -- bench.py's process, every leg after a three-group batch at full speed -- and worth
     *  6 % at 32 frames, 3 % at 64.) */
    /* Round 6 (the advisor's finding on round 5): three is OPT-IN -- pngloss_hip_set_option(ctx, "launch_groups", "3"), for a process that uses the synchronous
     * entry point only (bench.py's batch legs do and say so in their output) --, because nothing stopped a process from running a three-group batch and an asynchronous
     * one with a stream of its own later: the default is two.  Two guards on top, process-wide: once ANY context of the process has put a wait on a caller's stream no
     * third engine stream is created any more (stream_wait_used); and once a third engine stream exists the asynchronous entry takes its blocking variant (no wait on any
     * stream) instead of running at half speed behind one (run_seg_engine). */
    const bool three = in.opt_launch_groups == 3 && in.sync_call && in.three_groups_ok && n_seg >= 12 && !in.stream_wait_used;
    int ngroups = 1;
    if (segs > SEG_UNIT_MIN_SEGS && n_seg >= 8) ngroups = three ? 3 : 2;
    else if (n_seg >= 2) ngroups = 2;                              /* (a small batch: see the shares below) */
    if (hk.seg_groups) ngroups = hk.seg_groups;                    /* (timing / test hook: results do not depend on it) */
    ngroups = (int)std::min<size_t>((size_t)ngroups, n_seg);
    p.ngroups = ngroups;
    /* group g = images [gfirst[g], gfirst[g + 1]) of the list: equal shares -- or, in a batch of two groups whose tallest image stands out, that
     * image alone and the others together.  A group takes as many attempts as its image with the most, and every attempt costs what ALL its images' workgroups
     * cost: the reference's suite as one batch (configs[2]) spent 71 ms on the 1199 attempts of its tallest image, a screenshot whose candidate none fails in 40 % of
     * its rows -- at the price of eight images each; the other seven need 625 (profiles/r05_suite_groups.txt). */
    for (int g = 0; g <= ngroups; g++) p.gfirst[g] = n_seg * (size_t)g / (size_t)ngroups;
    if (ngroups == 2 && n_seg > 2 && !hk.seg_groups) {
        const uint32_t h0 = H[list[0]], h1 = H[list[1]];
        if ((uint64_t)h0 * 100u > (uint64_t)h1 * 105u) p.gfirst[1] = 1;
    }

    p.kind = pl_enum_kind(segs, n_seg, sp, hk.seg_unit, hk.seg_seeds, hk.seg_seeds1);
    const bool units = pl_enum_in_units(p.kind);
    sp.unit = units ? SEG_UNIT : 1;
    sp.tparts = units ? SEG_TPARTS_BATCH : SEG_TPARTS;     /* (batches: one control workgroup per candidate) */
    if (hk.tparts == 1 || hk.tparts == SEG_TPARTS) sp.tparts = hk.tparts == 1 ? SEG_TPARTS_BATCH : SEG_TPARTS;   /* (timing / test hook) */
    if (hk.seed_kin >= 1 && hk.seed_kin <= SEG_SEED_KMAX) sp.seed_kin = hk.seed_kin;   /* (timing hook) */
    if (in.forced_filter >= 0) sp.engine_flags = (in.forced_filter + 1) << 8;          /* (debugging build only) */
    if (hk.segprof) sp.engine_flags |= 1;                                               /* phase clocks of the validation kernel */
    if (sp.seeded && hk.kin >= 0 && hk.kin <= SEG_KIN) sp.kin = hk.kin;                 /* experiment: run-in pixels of the seeded enumeration */

    uint32_t max_h = 0;
    for (int g = 0; g < ngroups; g++) {
        PlSegGroupPlan &b = p.group[g];
        b.n = p.gfirst[g + 1] - p.gfirst[g];
        for (size_t i = p.gfirst[g]; i < p.gfirst[g + 1]; i++) {
            const uint32_t w = W[list[i]];
            const PlSegLayout l = pl_seg_layout(w ? w : 1, (uint32_t)sp.nsp, sp.seeded != 0);
            b.max_nseg = std::max(b.max_nseg, l.nseg); b.max_ngrp = std::max(b.max_ngrp, l.ngrp);
            b.max_ncommit = std::max(b.max_ncommit, (w + SEG_COMMIT_W - 1) / SEG_COMMIT_W);
            max_h = std::max(max_h, H[list[i]]);
        }
        if (!b.max_ncommit) b.max_ncommit = 1;
        b.small_ok = sp.small_ok != 0;
        b.seeded = sp.seeded != 0;
        b.unit = (uint32_t)sp.unit;
        b.seeds = pl_enum_from_seeds(p.kind);
        b.tparts = (uint32_t)sp.tparts;
        b.enum_nt = (size_t)b.max_nseg * b.n <= SEG_ENUM_NT_SMALL_MAX_NSEG ? 512u : 1024u;     /* (the images of THIS group: gridDim.y of its launches) */
        if (hk.enum_nt == 512 || hk.enum_nt == 1024) b.enum_nt = (uint32_t)hk.enum_nt;   /* test hook */
    }
    p.max_attempts = pl_seg_max_attempts(max_h, sp.strength);
    return p;
}

/* ---- a window of host images in chunks, each on its own context of the device (batch_host) --------------------------------------------------------------------
 * Chunk k+1 is staged and uploaded while chunk k computes, chunk k is downloaded while chunk k+1 computes.  Measured on 256 x 1280x720 (profiles/r03_host_seam.txt):
 * one chunk 0.237 s, two 0.221 s, four 0.218 s (the engine alone: 0.176 s) -- two it is; PNGLOSS_HIP_SPLIT=k for experiments.  A window with a deflate stage keeps
 * its single pass (it sorts the whole window's scanlines as one stream). */
inline size_t pl_host_window_chunks(size_t n, const PlHooks &hk, bool deflate)
{
    size_t K = n >= 16 ? 2 : 1;
    if (hk.split) K = (size_t)hk.split;
    if (K > n) K = n ? n : 1;
    return (deflate || hk.no_split) ? 1 : K;
}
/* first[c] = the first image of chunk c of K (first[K] = n): cut where the pixels are, equal shares */
inline std::vector<size_t> pl_host_window_cut(const std::vector<uint64_t> &pixels, size_t K)
{
    const size_t n = pixels.size();
    size_t total = 0;
    for (size_t i = 0; i < n; i++) total += pixels[i];
    std::vector<size_t> first(K + 1, n);
    first[0] = 0;
    size_t run = 0, c = 1;
    for (size_t i = 0; i < n && c < K; i++) {
        run += pixels[i];
        if (run * K >= total * c && i + 1 < n) first[c++] = i + 1;
    }
    for (; c < K; c++) first[c] = n;
    return first;
}

#endif

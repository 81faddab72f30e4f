/*
 * pl_seg_launch.h -- the SHAPE of a row attempt of the segment engine, stated once: which kernels an attempt launches, with what grid, workgroup size,
 * LDS bytes and scalar arguments (seg_attempt_launches), and what each workgroup of such a grid does (seg_dispatch_*: the inverse arithmetic, the early
 * returns, the call of the kernel body in pl_seg_core.h).  Internal.
 *
 * Plain C++17 plus the PLS_* macros of pl_seg_core.h, no HIP API.  pl_seg.hip carries it out -- its __global__ functions call the dispatch functions with
 * blockIdx.x and the launch's grid_x, its launcher loops over seg_attempt_launches() --, pl_plan.h fills the SegShape of every launch group, and the CPU harness
 * (tests/c/seg_host.cpp) runs the same launches block by block, so that the CPU suite covers the grids and the decode of the shipped library, not a copy of them
 * (tests/test_seg_launch_host.py pins every number and checks that every piece of work is visited exactly once).
 */
#ifndef PL_SEG_LAUNCH_H
#define PL_SEG_LAUNCH_H

#include "pl_seg_core.h"

#ifndef SEG_EXPERIMENT_NO_VAL_CODE
#define SEG_EXPERIMENT_NO_VAL_CODE 0      /* (1: TIMING EXPERIMENT -- the control kernel without the validation's code in it; results unvalidated) */
#endif
#ifndef SEG_BODY
#define SEG_BODY(name) name               /* (tests/c/seg_launch_host.cpp puts recording stubs in the bodies' place) */
#endif

/* what the attempts of a launch group depend on (pl_plan_batch fills it; the widest image of the group sets the three maxima) */
struct SegShape {
    uint32_t max_nseg, max_ngrp, max_ncommit;
    uint32_t enum_nt;         /* threads of the enumeration's workgroups: 512 or 1024 (SEG_ENUM_NT_SMALL_MAX_NSEG) */
    uint32_t tparts;          /* SegParams::tparts */
    uint32_t unit;            /* SegParams::unit: 1, or SEG_UNIT = enumeration in units (seg_k_enum_unit; batches) */
    bool small_ok;            /* SegParams::small_ok (none / up enumerated with their own small state set) */
    bool seeded;              /* SegParams::seeded (seg_k_enum_seeded) */
    bool seeds;               /* the units (or, unit = 1, the segments) may start from seeds with a run-in instead of from every state (SegParams::seed_n > 0; seg_unit_from_seeds decides per image, candidate and attempt) */
};

/* one value per kernel instantiation of pl_seg.hip */
enum SegKernel {
    SEG_KERNEL_CTL, SEG_KERNEL_CTL_BATCH,                          /* seg_k_ctl<SEG_TPARTS>, <SEG_TPARTS_BATCH> */
    SEG_KERNEL_ENUM_512, SEG_KERNEL_ENUM_1024,                     /* seg_k_enum<NT> */
    SEG_KERNEL_ENUM_SEEDED_512, SEG_KERNEL_ENUM_SEEDED_1024,       /* seg_k_enum_seeded<NT> */
    SEG_KERNEL_ENUM_UNIT, SEG_KERNEL_ENUM_UNIT1,                   /* seg_k_enum_unit<SEG_UNIT>, <1> */
    SEG_KERNEL_GATHER_SEEDED,                                      /* seg_k_gather_seeded */
    SEG_KERNEL_CHAIN, SEG_KERNEL_CHAIN_SEEDED, SEG_KERNEL_CHAIN_UNIT,   /* seg_k_chain<false, SEG_CHAIN_THREADS, false>, <true, SEG_CHAIN_THREADS, false>, <false, SEG_CHAIN_THREADS_UNIT, true> */
    SEG_KERNEL_REPLAY, SEG_KERNEL_REPLAY_BATCH,                    /* seg_k_replay<SEG_REPLAY_NT>, <SEG_REPLAY_NT_BATCH> */
    SEG_KERNEL_COUNT
};

/* one launch of an attempt: grid (grid_x, images of the group), `threads` a workgroup, `lds_bytes` of dynamic LDS, and the kernel's scalar arguments behind `par`:
 * control a = nctl, b = max_ngrp; enumeration a = max_nseg (and grid_x, which its dispatch reads: no kernel reads gridDim) -- in units / from seeds a = perb, b = pers, seeds; gather a = nblk; chain none; replay a = max_ngrp */
struct SegLaunch {
    SegKernel kernel;
    unsigned grid_x, threads;
    size_t lds_bytes;
    unsigned a, b;
    int seeds;
};
#define SEG_MAX_LAUNCHES 5

/* The launches of one attempt, in order: [control + validation of the attempt before], enumerate, (seeded sets: gather,) chain, replay.  Returns their number. */
inline int seg_attempt_launches(const SegShape &s, SegLaunch out[SEG_MAX_LAUNCHES])
{
    int n = 0;
    auto put = [&](SegKernel k, unsigned grid_x, unsigned threads, size_t lds, unsigned a = 0, unsigned b = 0, int seeds = 0) { out[n++] = SegLaunch{ k, grid_x, threads, lds, a, b, seeds }; };
    const bool batch_ctl = s.tparts == SEG_TPARTS_BATCH, units = s.unit > 1, nt512 = s.enum_nt == 512;
    {
        /* (the validation workgroups can be left out at COMPILE time only -- SEG_EXPERIMENT_NO_VAL_CODE, a timing experiment whose results are unvalidated;
         *  the shipped library has no run-time switch that changes what it computes) */
        const unsigned nctl = SEG_NFILT * s.tparts + 1 + s.max_ncommit, nval = SEG_EXPERIMENT_NO_VAL_CODE ? 0u : SEG_NFILT * s.max_ngrp * (SEG_GRP / SEG_VGRP_OF(s.tparts));
        put(batch_ctl ? SEG_KERNEL_CTL_BATCH : SEG_KERNEL_CTL, nctl + nval, SEG_THREADS, batch_ctl ? seg_lds_ctl_bytes<SEG_TPARTS_BATCH>() : seg_lds_ctl_bytes<SEG_TPARTS>(), nctl, s.max_ngrp);
    }
    const unsigned nt = s.enum_nt, halves = 4 / (nt / SEG_NSP), small_segs = nt / (4 * SEG_NSS);
    if ((s.unit == 1 && s.seeds && !s.seeded) || (units && !s.seeded)) {
        /* through the unit enumeration's bodies: batches in units of SEG_UNIT segments -- or (round 6) small and mid-size batches segment by segment, from seeds.
         * perb workgroups per candidate for whichever of its two bodies takes fewer pairs each, pers for none / up with their small state set */
        const unsigned u = units ? SEG_UNIT : 1, pairs = ((s.max_nseg + u - 1) / u) * 4;
        const unsigned nc_seeds = SEG_UNC_SEEDS_OF(u), nc_min = s.seeds && nc_seeds < SEG_UNC ? nc_seeds : SEG_UNC, nc_small = SEG_UNC_SMALL_OF(u);
        const unsigned perb = (pairs + nc_min - 1) / nc_min, pers = (pairs + nc_small - 1) / nc_small;
        put(units ? SEG_KERNEL_ENUM_UNIT : SEG_KERNEL_ENUM_UNIT1, (s.small_ok ? 3 * perb + 2 * pers : SEG_NFILT * perb) + SEG_NFILT, SEG_UNT, seg_lds_unit_bytes(), perb, pers, s.seeds ? 1 : 0);
    } else if (s.seeded) {
        put(nt512 ? SEG_KERNEL_ENUM_SEEDED_512 : SEG_KERNEL_ENUM_SEEDED_1024, SEG_NFILT * s.max_nseg * halves + SEG_NFILT, nt512 ? 512 : 1024, seg_lds_seeded_bytes(nt), s.max_nseg);
    } else {
        const unsigned blocks = (s.small_ok ? 3 * s.max_nseg * halves + 2 * ((s.max_nseg + small_segs - 1) / small_segs) : SEG_NFILT * s.max_nseg * halves) + SEG_NFILT;
        put(nt512 ? SEG_KERNEL_ENUM_512 : SEG_KERNEL_ENUM_1024, blocks, nt512 ? 512 : 1024, seg_lds_enum_bytes(nt), s.max_nseg);
    }
    if (s.seeded && s.max_nseg > 1) {
        const unsigned nblk = (s.max_nseg - 1 + SEG_GS - 1) / SEG_GS;
        put(SEG_KERNEL_GATHER_SEEDED, SEG_NFILT * 4 * nblk, SEG_GT, 0, nblk);
    }
    if (s.seeded) put(SEG_KERNEL_CHAIN_SEEDED, SEG_NFILT * 4 + 1, SEG_CHAIN_THREADS, seg_lds_chain_bytes<true>(s.max_nseg));
    else if (units) put(SEG_KERNEL_CHAIN_UNIT, SEG_NFILT * 4 + 1, SEG_CHAIN_THREADS_UNIT, seg_lds_chain_bytes<false>((s.max_nseg + s.unit - 1) / s.unit));
    else put(SEG_KERNEL_CHAIN, SEG_NFILT * 4 + 1, SEG_CHAIN_THREADS, seg_lds_chain_bytes<false>(s.max_nseg));
    put(units ? SEG_KERNEL_REPLAY_BATCH : SEG_KERNEL_REPLAY, SEG_NFILT * s.max_ngrp, units ? SEG_REPLAY_NT_BATCH : SEG_REPLAY_NT, seg_lds_replay_bytes(), s.max_ngrp);
    return n;
}

/* ---- what workgroup bx of a grid of gx does: j = the image's record, already loaded; rec = where it lives (the view is read from there) ---------------------- */

/* a workgroup's view of attempt k (SegCtlView).  On the device straight from the record in device memory.  Every address follows from the kernel's arguments,
 * but these scalar loads do NOT travel with the loads of the record itself: the compiler requests a scalar load where its value is first needed and moves it
 * behind every branch it can (the `||` below is such a branch), so a kernel waits for the record's fields, for the view, and for `ignore` and the fail mask, one
 * round trip after another (profiles/seg_heads.txt).  Such a trip costs 0.06-0.1 us behind a kernel boundary (profiles/ubench_headtrips.txt), less than what
 * holding the words in scalar registers costs the enumeration, the chain and the control kernel (profiles/seg_heads.txt: measured, kernel by kernel), so they
 * keep this form.  WHOLE (the replay, where it does pay): all of v[k] and the fail mask, no load conditional -- its kernel pins them in front of its first
 * branch (pl_seg.hip: seg_k_replay), one burst with the record's fields and one wait before the first request for data. */
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) SegJob *seg_const_job;
struct SegViewWords { uint32_t finished, y, s, ignore, magic, active[SEG_NFILT], start_x[SEG_NFILT], fail; };
__device__ __forceinline__ SegViewWords seg_view_words(const SegJob *rec, int k)
{
    seg_const_job c = (seg_const_job)(uintptr_t)rec;
    SegViewWords w;
    w.finished = c->v[k].finished; w.y = c->v[k].y; w.s = c->v[k].s; w.ignore = c->v[k].ignore; w.magic = c->v[k].magic;
    for (int f = 0; f < SEG_NFILT; f++) { w.active[f] = c->v[k].active[f]; w.start_x[f] = c->v[k].start_x[f]; }
    w.fail = c->vfail[seg_k_prev(k)];
    return w;
}
/* seg_head_pin(x, ..) wants its arguments in scalar registers at the place where it stands and emits nothing: in front of a kernel's first branch it keeps
 * their loads there, unconditional (all arguments are evaluated -- requested -- before the first of them is pinned) */
template <typename T> __device__ __forceinline__ void seg_head_pin1(T x) { asm volatile("" :: "s"(x)); }
template <typename... T> __device__ __forceinline__ void seg_head_pin(T... x) { (seg_head_pin1(x), ...); }
template <> __device__ __forceinline__ void seg_head_pin1(SegViewWords w)
{
    seg_head_pin(w.finished, w.y, w.s, w.ignore, w.magic, w.fail);
    for (int f = 0; f < SEG_NFILT; f++) seg_head_pin(w.active[f], w.start_x[f]);
}
#endif
template <bool WHOLE = false>
PLS_HD SegCtlView seg_view_of(const SegJob *rec, int k, int f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    SegCtlView v;
    if (WHOLE) {
        static_assert(SEG_NFILT == 5, "the selects below");
        const SegViewWords w = seg_view_words(rec, k);
        v.y = w.y; v.s = w.s;
        v.active = f == 0 ? w.active[0] : f == 1 ? w.active[1] : f == 2 ? w.active[2] : f == 3 ? w.active[3] : w.active[4];
        v.start_x = f == 0 ? w.start_x[0] : f == 1 ? w.start_x[1] : f == 2 ? w.start_x[2] : f == 3 ? w.start_x[3] : w.start_x[4];
        v.finished = (unsigned)(w.finished != 0u) | (unsigned)(w.magic != SEG_MAGIC) | (unsigned)((w.fail & ~w.ignore) != 0u);
        return v;
    }
    seg_const_job c = (seg_const_job)(uintptr_t)rec;
    const uint32_t fin = c->v[k].finished, magic = c->v[k].magic, ign = c->v[k].ignore, fm = c->vfail[seg_k_prev(k)];
    v.y = c->v[k].y; v.s = c->v[k].s; v.active = c->v[k].active[f]; v.start_x = c->v[k].start_x[f];
    v.finished = (fin != 0u || magic != SEG_MAGIC || (fm & ~ign) != 0u) ? 1u : 0u;
    return v;
#else
    return seg_ctl_view(*rec, k, f);
#endif
}

/* First launch of attempt k: its CONTROL workgroups (bx < nctl: decide the attempt before optimistically, commit, prepare this one -- SEG_NFILT * TPARTS candidate
 * workgroups, the image-wide one, the commit workgroups) and, side by side with them, the VALIDATION workgroups of the attempt before: the proof of what is being
 * decided arrives one launch later and takes nothing off the critical path (seg_ctl_body says what happens when it fails). */
template <int TPARTS>
PLS_HD void seg_dispatch_ctl(const SegJob &j, const SegJob *rec, const SegParams &P, int k, unsigned nctl, unsigned max_ngrp, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)gx;
    if (bx < nctl) {
        constexpr unsigned ctl_img = SEG_NFILT * TPARTS;
        if (bx > ctl_img && (bx - ctl_img - 1) * SEG_COMMIT_W >= j.W) return;
        SEG_BODY(seg_ctl_body)<TPARTS>(j, P, k, (int)bx, smem);
        return;
    }
#if SEG_EXPERIMENT_NO_VAL_CODE
    return;
#endif
    /* validation groups are half replay groups (one image) or whole ones (batches in units): max_ngrp * (SEG_GRP / VGRP) workgroups per candidate */
    constexpr unsigned VGRP = SEG_VGRP_OF(TPARTS);
    const unsigned r = bx - nctl, per = max_ngrp * (SEG_GRP / VGRP), f = r / per, vg = r % per;
    if (vg * VGRP >= j.nseg) return;
    SEG_BODY(seg_post_body)<(int)VGRP>(j, P, seg_view_of(rec, seg_k_prev(k), (int)f), seg_k_prev(k), (int)f, (int)vg, smem);
}

/* NT threads per workgroup: 1024 (four channels of a segment) or 512 (a channel pair), see SEG_ENUM_NT_SMALL_MAX_NSEG.
 * workgroups [0, nbig * max_nseg * halves): one segment (and channel group) of a filter that looks at the left pixel; behind them:
 * NT / 128 segments of none / up each; the last five walk the epoch's first segment of one candidate each */
template <int NT>
PLS_HD void seg_dispatch_enum(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned max_nseg, unsigned bx, unsigned gx, unsigned char *smem)
{
    const bool small_ok = P.small_ok != 0;
    const unsigned nbig = small_ok ? 3u : 5u;
    constexpr unsigned halves = 4 / (NT / SEG_NSP), small_segs = NT / (4 * SEG_NSS);
    if (bx < nbig * max_nseg * halves) {
        const unsigned k = bx / (max_nseg * halves), r = bx % (max_nseg * halves), seg = r / halves, chalf = r % halves;
        /* The candidates in the order paeth, avg, (up,) sub, (none): the LONGEST first.  The workgroups of a launch are handed out in the order of blockIdx, a CU of the
         * headline row gets one of each candidate, and a SIMD issues for its oldest waves first: in the phase in which all eight waves of every workgroup step (the
         * first steps and the dedupe) the workgroup dispatched last waits for the other two -- 3.4 / 4.0 / 5.9 us for the first / second / third of a CU, whichever
         * candidate it is.  With sub first and paeth last, the launch ended with paeth's workgroups (5.9 + its 5.7 us behind the dedupe); with paeth first it ends
         * with sub's, 1.1 us earlier (profiles/r11_enum_tail_placement.txt, table c): 14.60 -> 13.73 us a launch. */
        const unsigned f = small_ok ? (k == 0 ? 4u : (k == 1 ? 3u : 1u)) : 4u - k;
        if (seg >= j.nseg) return;
        SEG_BODY(seg_enum_body)<NT>(j, P, seg_view_of(rec, par, (int)f), par, (int)f, (int)seg, (int)chalf, smem);
    } else if (bx < gx - SEG_NFILT) {
        const unsigned r = bx - nbig * max_nseg * halves, per = (max_nseg + small_segs - 1) / small_segs;
        const unsigned f = r / per ? 2u : 0u, seg0 = (r % per) * small_segs;
        if (seg0 >= j.nseg) return;
        SEG_BODY(seg_enum_small_body)<NT>(j, P, seg_view_of(rec, par, (int)f), par, (int)f, (int)seg0, smem);
    } else {
        SEG_BODY(seg_first_body)<NT, false>(j, P, seg_view_of(rec, par, (int)(bx - (gx - SEG_NFILT))), par, (int)(bx - (gx - SEG_NFILT)), smem);
    }
}

/* seeded state sets (SegParams::seeded): every filter through seg_enum_seeded_body, one workgroup per (filter, segment, channel group); the
 * last five walk the epoch's first segment */
template <int NT>
PLS_HD void seg_dispatch_enum_seeded(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned max_nseg, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)gx;
    constexpr unsigned halves = 4 / (NT / SEG_NSP);
    if (bx < SEG_NFILT * max_nseg * halves) {
        const unsigned f = bx / (max_nseg * halves), r = bx % (max_nseg * halves), seg = r / halves, chalf = r % halves;
        if (seg >= j.nseg) return;
        SEG_BODY(seg_enum_seeded_body)<NT>(j, P, seg_view_of(rec, par, (int)f), par, (int)f, (int)seg, (int)chalf, smem);
    } else {
        SEG_BODY(seg_first_body)<NT, false>(j, P, seg_view_of(rec, par, (int)(bx - SEG_NFILT * max_nseg * halves)), par, (int)(bx - SEG_NFILT * max_nseg * halves), smem);
    }
}

/* enumeration in UNITS (batches; SegParams::unit = SEG_UNIT): first the filters that look at the left pixel (their workgroups are the long ones: `perb`
 * workgroups of SEG_UNC (unit, channel) pairs per candidate), then none / up -- with their small state set (when it exists) segment by segment, `pers`
 * workgroups of SEG_UNC_SMALL (unit, channel) pairs --, and the five walkers of an epoch's first unit.
 * `seeds` (round 6): the launcher offers the start from seeds (seg_unit_from_seeds decides per image, candidate and attempt); perb is then sized for whichever of the two
 * bodies needs more workgroups (seg_attempt_launches).
 * UNIT = SEG_UNIT: batches composed in units.  UNIT = 1 (round 6): the SAME bodies segment by segment -- (segment, channel) pairs, each started from
 * seeds eight pixels in front of it -- for small and mid-size batches, whose attempts are bound by the enumeration's dependent path, not by its work: 8 + 32 dependent
 * steps instead of 8 + 96, a twentieth of the workgroups of seg_k_enum (one per segment and channel pair, every segment from all 253 states). */
template <int UNIT>
PLS_HD void seg_dispatch_enum_unit(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned perb, unsigned pers, int seeds, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)gx;
    const bool small_ok = P.small_ok != 0;
    constexpr int NCS = SEG_UNC_SMALL_OF(UNIT);
    const unsigned nbig = small_ok ? 3u : 5u, nb = nbig * perb, ns = small_ok ? 2u * pers : 0u;
    if (bx >= nb + ns) {
        SEG_BODY(seg_first_body)<SEG_UNT, (UNIT > 1)>(j, P, seg_view_of(rec, par, (int)(bx - nb - ns)), par, (int)(bx - nb - ns), smem);
        return;
    }
    const unsigned npairs = ((j.nseg + UNIT - 1) / UNIT) * j.bpp;
    if (bx < nb) {
        const unsigned k = bx / perb, grp = bx % perb;
        const unsigned f = small_ok ? (k == 0 ? 1u : (k == 1 ? 3u : 4u)) : k;
        const SegCtlView cv = seg_view_of(rec, par, (int)f);
        if (seeds && seg_unit_from_seeds(j, P, cv, (int)f, seeds)) {
            if (grp * SEG_UNC_SEEDS_OF(UNIT) >= npairs) return;
            SEG_BODY(seg_enum_unit_body)<SEG_SEED_LANES, UNIT, SEG_UNC_SEEDS_OF(UNIT), true>(j, P, cv, par, (int)f, (int)grp, smem);
            return;
        }
        if (grp * SEG_UNC >= npairs) return;
        SEG_BODY(seg_enum_unit_body)<SEG_NSP, UNIT, SEG_UNC>(j, P, cv, par, (int)f, (int)grp, smem);
    } else {
        const unsigned r = bx - nb, f = r / pers ? 2u : 0u, grp = r % pers;
        if (grp * NCS >= npairs) return;
        SEG_BODY(seg_enum_unit_body)<SEG_NSS, UNIT, NCS>(j, P, seg_view_of(rec, par, (int)f), par, (int)f, (int)grp, smem);
    }
}

/* seeded state sets: the dense transitions of the enumerated segments, between the enumeration and the chain (seg_gather_seeded_body); 5 x 4 x nblk workgroups */
PLS_HD void seg_dispatch_gather(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned nblk, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)P; (void)gx; (void)smem;
    const unsigned fc = bx / nblk, blk = bx % nblk;
    if (blk * SEG_GS + 1u >= j.nseg) return;
    SEG_BODY(seg_gather_seeded_body)(j, seg_view_of(rec, par, (int)(fc >> 2)), (int)(fc >> 2), (int)(fc & 3), (int)blk);
}

/* 5 x 4 chain workgroups (candidate, channel) behind the spare one, dispatched first: the row's extremes for none's bound */
template <bool SEEDED, int CT, bool UNITS>
PLS_HD void seg_dispatch_chain(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)gx;
    if (bx == 0) { SEG_BODY(seg_extremes_body)<CT>(j, P, seg_view_of(rec, par, 0), par, smem); return; }
    SEG_BODY(seg_chain_body)<SEEDED, CT, UNITS>(j, P, seg_view_of(rec, par, (int)((bx - 1) >> 2)), par, (int)((bx - 1) >> 2), (int)((bx - 1) & 3), smem);
}

template <int RNT>
PLS_HD void seg_dispatch_replay(const SegJob &j, const SegJob *rec, const SegParams &P, int par, unsigned max_ngrp, unsigned bx, unsigned gx, unsigned char *smem)
{
    (void)gx;
    const unsigned f = bx / max_ngrp, grp = bx % max_ngrp;
    if (grp >= j.ngrp) return;
    SEG_BODY(seg_replay_body)<RNT>(j, P, seg_view_of<true>(rec, par, (int)f), par, (int)f, (int)grp, smem);
}

#if !defined(__HIPCC__)
/* the CPU harnesses: workgroup bx of launch L (what pl_seg.hip's launcher hands to the kernel of that id, and the kernel to its dispatch function) */
inline void seg_dispatch_block(const SegLaunch &L, const SegJob &j, const SegParams &P, int par, unsigned bx, unsigned char *smem)
{
    const unsigned gx = L.grid_x;
    switch (L.kernel) {
    case SEG_KERNEL_CTL: seg_dispatch_ctl<SEG_TPARTS>(j, &j, P, par, L.a, L.b, bx, gx, smem); break;
    case SEG_KERNEL_CTL_BATCH: seg_dispatch_ctl<SEG_TPARTS_BATCH>(j, &j, P, par, L.a, L.b, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_512: seg_dispatch_enum<512>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_1024: seg_dispatch_enum<1024>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_SEEDED_512: seg_dispatch_enum_seeded<512>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_SEEDED_1024: seg_dispatch_enum_seeded<1024>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_UNIT: seg_dispatch_enum_unit<SEG_UNIT>(j, &j, P, par, L.a, L.b, L.seeds, bx, gx, smem); break;
    case SEG_KERNEL_ENUM_UNIT1: seg_dispatch_enum_unit<1>(j, &j, P, par, L.a, L.b, L.seeds, bx, gx, smem); break;
    case SEG_KERNEL_GATHER_SEEDED: seg_dispatch_gather(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_CHAIN: seg_dispatch_chain<false, SEG_CHAIN_THREADS, false>(j, &j, P, par, bx, gx, smem); break;
    case SEG_KERNEL_CHAIN_SEEDED: seg_dispatch_chain<true, SEG_CHAIN_THREADS, false>(j, &j, P, par, bx, gx, smem); break;
    case SEG_KERNEL_CHAIN_UNIT: seg_dispatch_chain<false, SEG_CHAIN_THREADS_UNIT, true>(j, &j, P, par, bx, gx, smem); break;
    case SEG_KERNEL_REPLAY: seg_dispatch_replay<SEG_REPLAY_NT>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_REPLAY_BATCH: seg_dispatch_replay<SEG_REPLAY_NT_BATCH>(j, &j, P, par, L.a, bx, gx, smem); break;
    case SEG_KERNEL_COUNT: break;
    }
}
#endif

#endif

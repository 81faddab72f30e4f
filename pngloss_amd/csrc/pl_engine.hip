/*
 * pl_engine.hip -- the row engine: pngloss's per-scanline optimiser as ONE persistent gfx950 kernel.
 *
 * Replaces, for a whole image, the reference's
 *     optimize_image            /root/reference/src/pngloss_image.c:159-333   (row loop, 5-filter search, retry, commit)
 *     optimize_state_row / _run /root/reference/src/optimize_state.c:292-361, 114-290
 *     diffuse_color_error       /root/reference/src/optimize_state.c:390-490
 *     adaptive_filter_for_rows  /root/reference/src/optimize_state.c:492-562
 *     color_delta.c             /root/reference/src/color_delta.c:4-66
 *
 * One workgroup = one image (blockIdx.x = image of the batch), 8 wavefronts, persistent over all rows.  The five candidate
 * filters of a row are independent (pngloss_image.c:213,240): waves 0..4 run their serial chains concurrently (up, sub,
 * average, paeth, none); all eight waves run the passes that are parallel over x (post pass, commit).
 *
 * Two formulations of the chain live here, both exact:
 *   band-leader chains (round 2, chain_lead: pl_wg_lead.h, DESIGN_APPENDIX.md section A): per pixel and channel ONE
 *     dependent LDS lookup in a decision table built from the leaders of the quantisation bands, hand-scheduled loops
 *     (pl_lead_asm.h) on four lanes, histogram bumps deferred and applied 64 pixels at a time under a rule that keeps the table
 *     true (watched relations), exceptions settled without the histogram where it cannot matter (light pixels) and by the
 *     round-1 evaluation otherwise;
 *   round-1 chains (chain_row: pl_wg_chain.h): lanes 16c..16c+15 = channel c of the current pixel (a DPP row) hold the <= s+1 candidate symbols
 *     of that channel's band (optimize_state.c:186-214); per pixel: predict -> re-centre -> band -> clamp, gather of {running
 *     frequency, rank of original frequency}, two DPP arg-max reductions of the reference's 4-level key, exact repair of the
 *     coupling between the channels of a pixel (optimize_state.c:221,253).  They take the rows the band-leader chains cannot
 *     (q > 128, exploding errors) and the rows where those are measurably slower (adaptive choice per row, from cycle counts).
 * The Sierra terms that feed the same row (x+1, x+2) ride in the table entries / registers; the eight terms for the next two
 * rows, the derivative error metric, libpng's heuristic and the entropy cost are deferred to the passes parallel over x.
 *
 * The x-chain and the row-to-row dependence through the winner's histogram are inherently serial (SURVEY.md
 * Appendix C): this kernel is bound by that dependency chain, not by HBM and not by MFMA.
 */
#include "pl_device.h"
#include "pl_wg_lds.h"

#include <atomic>
#include <cstdio>
#include <type_traits>

/* the stages of a row, in the order the kernel below goes through them (parts of this file: they share its anonymous namespace) */
namespace {

#include "pl_wg_util.h"    /* DPP / wave helpers, address-space typedefs */
#include "pl_wg_chain.h"   /* round-1 chains: RowCtx, chain_row, chain_dispatch */
#include "pl_wg_lead.h"    /* band-leader chains: band geometry, tables, rescan, exact pixel, fast run, chain_lead, chain_lead_dispatch */
#include "pl_wg_post.h"    /* post pass: post_pass_all */

} // namespace

#ifndef PL_POST_EARLY
#define PL_POST_EARLY 2u        /* how many of the first chains to finish do their own candidate's post pass (0: none) */
#endif
#ifndef PL_ADAPT_SLOW
#define PL_ADAPT_SLOW 600u      /* band-leader rows slower than this many cycles per pixel make the kernel try the round-1 chains */
#endif
#ifndef PL_ADAPT_REPROBE
#define PL_ADAPT_REPROBE 32u
#endif

__global__ __launch_bounds__(PL_ENGINE_THREADS) void pl_engine(const PlJob *jobs, const uint32_t *sel, PlEngineParams prm)
{
    /* LDS (dynamic: the band-leader tables push the total past the 64 KB static limit; gfx950 has 160 KB).  The carve-up is pl_wg_lds.h's table: every offset
     * below is a compile-time constant out of it */
    extern __shared__ __align__(16) unsigned char smem_raw[];
    /* the histogram tables sit 4 KB aligned (the band-leader chain ORs the bin offset into the table address): PL_WG_ALIGN_SLACK pays for the rounding */
    unsigned char *const smem = smem_raw + ((PL_TBL_ALIGN - ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem_raw & (PL_TBL_ALIGN - 1u))) & (PL_TBL_ALIGN - 1u));
    uint2 (*const tbl)[PL_TBL_N] = (uint2 (*)[PL_TBL_N])(smem + PL_WG_OFF(TBL));
    uint32_t *const Hc = (uint32_t *)(smem + PL_WG_OFF(HC));
    uint32_t *const split_lut = (uint32_t *)(smem + PL_WG_OFF(SPLIT_LUT));
    uint32_t *const split_lut2 = (uint32_t *)(smem + PL_WG_OFF(SPLIT_LUT2));
    unsigned long long *const costs = (unsigned long long *)(smem + PL_WG_OFF(COSTS));
    uint32_t *const pacc = (uint32_t *)(smem + PL_WG_OFF(PACC));
    uint32_t *const flags = (uint32_t *)(smem + PL_WG_OFF(FLAGS));
    uint32_t &big_err = flags[PL_WG_F_BIG_ERR], &big_lead = flags[PL_WG_F_BIG_LEAD], &uniq = flags[PL_WG_F_UNIQ], &simd_map = flags[PL_WG_F_SIMD_MAP];
    uint32_t &chains_done = flags[PL_WG_F_CHAINS_DONE], &post_done = flags[PL_WG_F_POST_DONE], &rowcyc = flags[PL_WG_F_ROWCYC];
    /* the union: the round-1 chains' records, or the band-leader chains' decision tables, band states, work arrays, chain records and result rings (or the
     * commit pass's tterms, below) */
    uint4 *const rec = (uint4 *)(smem + PL_WG_OFF(REC));
    uint2 *const ltab = (uint2 *)(smem + PL_WG_OFF(LTAB));
    uint32_t *const lbs = (uint32_t *)(smem + PL_WG_OFF(LBS));
    uint32_t *const lwork = (uint32_t *)(smem + PL_WG_OFF(LWORK));
    unsigned char *const lrec = smem + PL_WG_OFF(LREC);
    uint2 *const lout = (uint2 *)(smem + PL_WG_OFF(LOUT));

    const PlJob j = jobs[sel ? sel[blockIdx.x] : blockIdx.x];   /* (sel: the images of a mixed batch that take this engine) */
    const uint32_t W = j.width, H = j.height;
    const uint32_t bpp = pl_job_bpp(j);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float r29 = 2.0f * __uint_as_float(__float_as_uint(1.0f / 9.0f) + 1u);

    for (int i = tid; i < PL_NSYM; i += PL_ENGINE_THREADS) Hc[i] = 0;
    for (int i = tid; i < PL_NFILT * PL_NSYM; i += PL_ENGINE_THREADS)
        tbl[i >> 8][i & 255] = make_uint2(0u, j.orig_rank[i] << 9);
    for (int i = tid; i < PL_NFILT * PL_TBL_DUMMY; i += PL_ENGINE_THREADS) tbl[i >> 6][PL_NSYM + (i & (PL_TBL_DUMMY - 1))] = make_uint2(0u, 0u);
    for (int i = tid; i < 512; i += PL_ENGINE_THREADS) {
        const PlSplit sp = pl_sierra_split(i - 256, prm.rbleed, r29);
        split_lut[i] = ((uint32_t)(int)sp.rem & 0xffffu) | ((uint32_t)(int)sp.h << 16);
        split_lut2[i] = ((uint32_t)(int)sp.t & 255u) | (((uint32_t)(int)sp.f & 255u) << 8) | (((uint32_t)(int)sp.v & 255u) << 16) | ((uint32_t)(int)sp.h << 24);
    }
    if (tid == 0) { big_err = 0; big_lead = 0; simd_map = 0; }
    __syncthreads();

    uint32_t retried = 0, slow_px = 0, light_px = 0, lead_rows = 0, lead_rebuilds = 0;
    /* Which chains a row takes where both could: the band-leader chains unless the rows they just did were slow (dense slow pixels:
     * noise with ties everywhere, transparency patterns) AND the round-1 chains, tried on one row, were faster.  Both are exact, so
     * the choice -- made from cycle counts -- never shows in the results.  est_*: cycles per pixel of the slowest chain wave of
     * the last row each kind ran (0 = not known); the loser is tried again every PL_ADAPT_REPROBE rows. */
    uint32_t est_lead = 0, est_legacy = 0, adapt_since = 0, adapt_legacy_rows = 0;
    bool use_legacy = false, adapt_prev_lead = true, adapt_was_legacy = false;
    uint32_t adapt_backoff = 2u, adapt_last_lead = ~0u;
    unsigned long long lead_cyc[PL_LC_N] = { 0, 0, 0, 0, 0, 0, 0, 0 };   /* diagnostics: PL_LC_* */
    unsigned long long cyc_post = 0, cyc_commit = 0;      /* diagnostics */
    unsigned long long chain_cycles = 0;
    int status = 0;
    for (uint32_t y = 0; y < H && !status; y++) {
        const bool adaptive = !j.row_filters || y == 0;   /* pngloss_image.c:210 */
        int s = prm.strength;
        int winner = -1;
        const bool wrap = big_err != 0 || prm.force_careful;
        for (;;) {
            /* every candidate starts from the committed histogram (optimize_state_copy, pngloss_image.c:240) */
            for (int i = tid; i < PL_NFILT * PL_NSYM; i += PL_ENGINE_THREADS) tbl[i >> 8][i & 255].x = Hc[i & 255];
            for (int i = tid; i < PL_NFILT * PL_PA_WORDS; i += PL_ENGINE_THREADS) pacc[i] = 0u;
            if (tid == 0) { rowcyc = 0u; chains_done = 0u; post_done = 0u; }
            __syncthreads();
            /* chain phase.  Band-leader chains (round 2): five waves, one per candidate filter -- their fast path has
             * no DPP, and plain VALU/LDS waves sharing a SIMD do not slow each other (profiles/r01_ubench_simd_sharing.txt).
             * Rows that do not meet its preconditions take the round-1 chains below. */
            const bool lead_ok = (prm.engine_mode & 15) != 1 && s + 1 <= 128 && !wrap && big_lead == 0;
            /* engine_mode 3 ("mix", a test hook): the two kinds of chains take turns every four rows, whatever the clocks say -- the
             * adaptive choice (mode 0) depends on measured cycles and would not reproduce a mismatch of one of them */
            if (lead_ok && (prm.engine_mode & 15) == 3) use_legacy = ((y >> 2) & 1u) != 0u;
            const bool lead = lead_ok && !(use_legacy && ((prm.engine_mode & 15) == 0 || (prm.engine_mode & 15) == 3));
            if ((prm.engine_mode & 15) == 3 && lead_ok && !lead) adapt_legacy_rows++;
            const int lead_f = wave == 0 ? 2 : (wave == 1 ? 1 : (wave == 2 ? 3 : (wave == 3 ? 4 : 0)));   /* up | sub | average | paeth | none */
            const bool paired = s + 1 <= 48;
            if (lead) {
              if (wave < PL_NFILT) {
                LeadCtx k;
                k.row = j.img + (size_t)y * W;
                k.nabove = y ? k.row - W : nullptr;
                k.err0 = j.err0;
                k.cand = j.cand + (size_t)lead_f * W;
                k.tbl = (lds_uint2 *)&tbl[lead_f][0];
                k.T = (lds_uint2 *)(ltab + pl_wg_lead_table(lead_f) * PL_LT_N);   /* none: tables 0 (P pixels) and 1 (N pixels) */
                k.bs = (lds_u32 *)(lbs + lead_f * (PL_WG_SLOT(LBS) / 4));
                k.work = (lds_u32 *)lwork + lead_f * PL_LWORK_N;
                k.crec = (lds_uint4 *)(lrec + lead_f * PL_WG_SLOT(LREC));   /* none, sub, up, average, paeth (two slots) */
                k.out = (lds_uint2 *)(lout + lead_f * (PL_WG_SLOT(LOUT) / PL_LOUT_BYTES));
                k.lut = (lds_u32 *)&split_lut[0];
                k.W = W; k.bpp = bpp; k.s = s; k.rq = recip_up(s + 1);
                k.slow = 0; k.rebuilds = 0; k.light = 0;
                const unsigned long long t0 = __builtin_readcyclecounter();
                lead_build_table(k, lead_geo(s, lead_f == 0, k.rq), lane);
                const unsigned long long tb1 = __builtin_readcyclecounter();
                switch (lead_f) {
                case 0: chain_lead_dispatch<0>(k, lane); break;
                case 1: chain_lead_dispatch<1>(k, lane); break;
                case 2: chain_lead_dispatch<2>(k, lane); break;
                case 3: chain_lead_dispatch<3>(k, lane); break;
                default: chain_lead_dispatch<4>(k, lane); break;
                }
                const unsigned long long dtc = __builtin_readcyclecounter() - t0;
                chain_cycles += dtc;
                if (lane == 0) atomicMax(&rowcyc, (uint32_t)min(dtc, 0xffffffffull));
#if PL_POST_EARLY
                {   /* the first chains to finish (usually up and none, well ahead of sub / average / paeth) do the post pass of their
                     * own candidate while the others still run: that much less for the joint pass behind the barrier */
                    uint32_t order = 0;
                    if (lane == 0) order = atomicAdd(&chains_done, 1u);
                    order = (uint32_t)__builtin_amdgcn_readfirstlane((int)order);
                    if (order < PL_POST_EARLY) {
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      /* this wave's candidate row is complete and visible to itself */
                        post_pass_all(j, y, bpp, tbl, adaptive, tid, pacc, (uint32_t)lane, 64u, 1u << lead_f);
                        if (lane == 0) atomicOr(&post_done, 1u << lead_f);
                    }
                }
#endif
                slow_px += k.slow;
                light_px += k.light;
                lead_rebuilds += k.rebuilds;
                lead_rows++;
                for (int qq = 0; qq <= PL_CC_RESCAN; qq++) lead_cyc[qq] += k.cyc[qq];   /* vector, fast, exact, rescan: the same positions in both */
                lead_cyc[PL_LC_BUILD] += tb1 - t0;
                lead_cyc[PL_LC_CLEAN] += k.cyc[PL_CC_CLEAN]; lead_cyc[PL_LC_CLEAN_PX] += k.cyc[PL_CC_CLEAN_PX]; lead_cyc[PL_LC_FLUSH] += k.cyc[PL_CC_FLUSH];
              }
            } else
            /* round-1 chains: four waves on the four SIMDs -- wave 0 runs the 'none' and 'up' chains side by side,
             * waves 1..3 run sub, average, paeth; wave 4 only takes part in the data-parallel passes */
            /* wide bands (s > 47) would need > 6 candidates per lane in the paired wave: there the five chains run as
             * five waves instead (wave 4 = 'up'), accepting that two of them share a SIMD */
            if (wave < PL_NFILT && (wave < 4 || !paired)) {
                RowCtx k;
                k.row = j.img + (size_t)y * W;
                k.nabove = y ? k.row - W : nullptr;
                k.err0 = j.err0;
                k.cand = j.cand;
                k.tbl = (lds_uint2 *)&tbl[0][0];
                k.rec = (lds_uint4 *)&rec[pl_wg_round1_slot(wave) * (PL_WG_SLOT(REC) / 16)];
                k.lut = (lds_u32 *)&split_lut[0];
                k.W = W; k.y = y; k.bpp = bpp; k.s = s;
                k.rq = recip_up(s + 1); k.rbleed = prm.rbleed; k.r29 = r29;
                k.slow = 0;
                const unsigned long long t0 = __builtin_readcyclecounter();
                switch (wave) {
                case 0: if (paired) chain_dispatch<5>(k, lane, wrap); else chain_dispatch<0>(k, lane, wrap); break;
                case 1: chain_dispatch<1>(k, lane, wrap); break;
                case 2: chain_dispatch<3>(k, lane, wrap); break;
                case 3: chain_dispatch<4>(k, lane, wrap); break;
                default: chain_dispatch<2>(k, lane, wrap); break;
                }
                const unsigned long long dtc = __builtin_readcyclecounter() - t0;
                chain_cycles += dtc;
                if (lane == 0) atomicMax(&rowcyc, (uint32_t)min(dtc, 0xffffffffull));
                slow_px += k.slow;
            }
            __syncthreads();   /* candidate rows (global, same CU) and histograms (LDS) complete and visible */
            if (lead_ok && (prm.engine_mode & 15) == 0) {
                const uint32_t pp = rowcyc / W + 1u;
                /* (band-leader rows: the faster of the last two, so that a single slow row -- they exist, 7x the average -- is not a reason to switch) */
                if (lead) { est_lead = adapt_prev_lead ? min(pp, adapt_last_lead) : pp; adapt_last_lead = pp; }
                else { est_legacy = (!adapt_prev_lead && est_legacy) ? (est_legacy + pp) >> 1 : pp; adapt_legacy_rows++; }

                adapt_prev_lead = lead;
                if (est_lead <= PL_ADAPT_SLOW) { use_legacy = false; adapt_since = 0; adapt_backoff = 2u; }
                else if (est_legacy == 0) use_legacy = true;                       /* first try of the round-1 chains */
                else {
                    /* The loser runs a row now and then.  While the round-1 chains win, the band-leader chains are tried again after
                     * 2, 4, 8 .. PL_ADAPT_REPROBE rows (a single slow row must not cost 32 rows of the slower engine; a slow region
                     * is probed rarely); the round-1 chains are retried every PL_ADAPT_REPROBE rows when close behind, else rarely. */
                    const bool legacy_better = 21u * est_legacy < 20u * est_lead;
                    if (lead && legacy_better && adapt_was_legacy) adapt_backoff = min(2u * adapt_backoff, PL_ADAPT_REPROBE);   /* a probe lost */
                    const uint32_t every = legacy_better ? adapt_backoff : (10u * est_legacy < 13u * est_lead ? PL_ADAPT_REPROBE : 256u);
                    if (++adapt_since >= every) { use_legacy = !legacy_better; adapt_since = 0; }
                    else use_legacy = legacy_better;
                }
                adapt_was_legacy = !lead;
            }
            const unsigned long long tpp0 = __builtin_readcyclecounter();
            /* post pass: all threads, all candidates (the accumulators were zeroed before the chain phase) */
            post_pass_all(j, y, bpp, tbl, adaptive, tid, pacc, (uint32_t)tid, PL_ENGINE_THREADS, 31u & ~post_done);
            cyc_post += __builtin_readcyclecounter() - tpp0;
            __syncthreads();
            if (tid < PL_NFILT) {
                const uint32_t *a8 = pacc + PL_PA_WORDS * tid;
                uint64_t cst = (((uint64_t)a8[PL_PA_DERR + 1] << 32) | a8[PL_PA_DERR]) / 128u + a8[PL_PA_COST];
                if (adaptive) {
                    int bestg = 0;
#pragma unroll
                    for (int g = 1; g < PL_NFILT; g++) if (a8[PL_PA_HS + g] < a8[PL_PA_HS + bestg]) bestg = g;
                    if (bestg != tid) cst = ~0ull;           /* libpng's heuristic would not have picked this filter (optimize_state.c:319-324) */
                }
                costs[tid] = (prm.engine_mode >> 8) ? (tid == (prm.engine_mode >> 8) - 1 ? 0ull : ~0ull) : cst;   /* debugging aid: force one candidate */
            }
            __syncthreads();
            uint64_t best = ~0ull;
#pragma unroll
            for (int f = 0; f < PL_NFILT; f++) {
                const uint64_t cf = costs[f];
                if (cf < best) { best = cf; winner = f; }     /* strict <: lowest filter index wins ties (pngloss_image.c:257) */
            }
            __syncthreads();
            if (winner >= 0) break;
            if (s == 0) { status = 65; break; }                /* pngloss_image.c:268-271 aborts here */
            s--;                                               /* pngloss_image.c:274 */
            retried += (s == prm.strength - 1);
        }
        if (status) break;

        /* ---- commit (pngloss_image.c:277-308), parallel over x ---- */
        const unsigned long long tcm0 = __builtin_readcyclecounter();
        if (tid == 0) { big_err = 0; big_lead = 0; }
        __syncthreads();
        bool big = false, bigl = false;
        const uint4 *__restrict__ cd = j.cand + (size_t)winner * W;
        uint32_t *__restrict__ rowp = j.img + (size_t)y * W;
        uint32_t *__restrict__ oldab = j.old_above;
        uint2 *__restrict__ perr0 = j.err0, *__restrict__ perr1 = j.err1;
        const uint32_t keep = bpp >= 4 ? 0xffffffffu : ((1u << (8 * bpp)) - 1u);
        /* next-rows Sierra terms of one pixel and channel (optimize_state.c:446-465): t | f << 8 | v << 16 | h << 24 (int8 each) from the
         * 512-entry LDS table of the split for |diff| <= 255, else by the float arithmetic of pl_sierra_split */
        auto terms_of = [&](const uint4 v, const int ch) -> uint32_t {
            const uint32_t w = ch == 0 ? v.x : (ch == 1 ? v.y : (ch == 2 ? v.z : v.w));
            const int diff = pl_sext16((int)(w >> 8));
            if (diff >= -256 && diff <= 255) return split_lut2[diff + 256];
            const PlSplit sp = pl_sierra_split(diff, prm.rbleed, r29);
            return ((uint32_t)(int)sp.t & 255u) | (((uint32_t)(int)sp.f & 255u) << 8) | (((uint32_t)(int)sp.v & 255u) << 16) | ((uint32_t)(int)sp.h << 24);
        };
        const auto T_ = [](uint32_t e) { return __builtin_amdgcn_sbfe((int)e, 0, 8); };
        const auto F_ = [](uint32_t e) { return __builtin_amdgcn_sbfe((int)e, 8, 8); };
        const auto V_ = [](uint32_t e) { return __builtin_amdgcn_sbfe((int)e, 16, 8); };
        const auto H_ = [](uint32_t e) { return (int)e >> 24; };
        if ((size_t)W * 16u <= (size_t)PL_WG_UNION_BYTES) {
            /* Two passes over the row through LDS (the chains' region is free now): every pixel's terms are looked up ONCE -- four
             * words, one per error plane -- and its four neighbours read them from there, instead of five pixels x four planes of
             * lookups per pixel. */
            uint4 *const tterms = (uint4 *)(smem + PL_WG_OFF(TTERMS));
#pragma unroll 4
            for (uint32_t x = tid; x < W; x += PL_ENGINE_THREADS) {
                const uint4 cw = cd[x];
                const uint32_t np = ((cw.x & 255u) | ((cw.y & 255u) << 8) | ((cw.z & 255u) << 16) | ((cw.w & 255u) << 24)) & keep;
                oldab[x] = rowp[x];
                rowp[x] = np;
                uint32_t tw[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int ch = pl_channel_of_plane(bpp, p);
                    tw[p] = ch >= 0 ? terms_of(cw, ch) : 0u;
                }
                tterms[x] = make_uint4(tw[0], tw[1], tw[2], tw[3]);
            }
            __syncthreads();
#pragma unroll 4
            for (uint32_t x = tid; x < W; x += PL_ENGINE_THREADS) {
                const uint2 e1 = perr1[x];
                const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);      /* (outside the row: diff 0, whose terms are 0) */
                const uint4 m2 = x >= 2 ? tterms[x - 2] : z4, m1 = x >= 1 ? tterms[x - 1] : z4, z0 = tterms[x];
                const uint4 p1 = x + 1 < W ? tterms[x + 1] : z4, p2 = x + 2 < W ? tterms[x + 2] : z4;
                const uint32_t am2[4] = { m2.x, m2.y, m2.z, m2.w }, am1[4] = { m1.x, m1.y, m1.z, m1.w }, az0[4] = { z0.x, z0.y, z0.z, z0.w };
                const uint32_t ap1[4] = { p1.x, p1.y, p1.z, p1.w }, ap2[4] = { p2.x, p2.y, p2.z, p2.w };
                uint32_t n0[4], n1[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const uint32_t e1p = p < 2 ? (e1.x >> (16 * p)) : (e1.y >> (16 * (p - 2)));
                    const int c1 = T_(ap2[p]) + F_(ap1[p]) + V_(az0[p]) + F_(am1[p]) + T_(am2[p]);
                    const int c2 = T_(ap1[p]) + H_(az0[p]) + T_(am1[p]);
                    n0[p] = (uint32_t)((int)e1p + c1) & 0xffffu;   /* int16 wrap-on-store */
                    big |= abs(pl_sext16((int)n0[p])) > 8000;
                    bigl |= abs(pl_sext16((int)n0[p])) > PL_E0_LEAD_MAX;
                    n1[p] = (uint32_t)c2 & 0xffffu;
                }
                perr0[x] = make_uint2(n0[0] | (n0[1] << 16), n0[2] | (n0[3] << 16));
                perr1[x] = make_uint2(n1[0] | (n1[1] << 16), n1[2] | (n1[3] << 16));
            }
        } else {
        /* (the pointers do not alias: telling the compiler lets it keep the loads of several iterations in flight) */
#pragma unroll 4
        for (uint32_t x = tid; x < W; x += PL_ENGINE_THREADS) {
            const uint4 cw = cd[x];
            const uint32_t np = ((cw.x & 255u) | ((cw.y & 255u) << 8) | ((cw.z & 255u) << 16) | ((cw.w & 255u) << 24)) & keep;
            oldab[x] = rowp[x];
            rowp[x] = np;
            const uint2 e1 = perr1[x];
            /* the five source pixels of the next-rows terms, loaded once for the four planes */
            const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
            const uint4 cm2 = x >= 2 ? cd[x - 2] : z4, cm1 = x >= 1 ? cd[x - 1] : z4;
            const uint4 cp1 = x + 1 < W ? cd[x + 1] : z4, cp2 = x + 2 < W ? cd[x + 2] : z4;
            uint32_t n0[4], n1[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int ch = pl_channel_of_plane(bpp, p);
                const uint32_t e1p = p < 2 ? (e1.x >> (16 * p)) : (e1.y >> (16 * (p - 2)));
                int c1 = 0, c2 = 0;
                if (ch >= 0) {
                    /* (rows wider than the LDS region: the five source pixels x-2..x+2 looked up per pixel) */
                    auto terms = [&](const uint4 v) -> uint32_t { return terms_of(v, ch); };
                    /* (a pixel outside the row has no record: all-zero words give diff 0, whose terms are 0) */
                    const uint32_t m2 = terms(cm2), m1 = terms(cm1), z0 = terms(cw), p1 = terms(cp1), p2 = terms(cp2);
                    c1 = T_(p2) + F_(p1) + V_(z0) + F_(m1) + T_(m2);
                    c2 = T_(p1) + H_(z0) + T_(m1);
                }
                n0[p] = (uint32_t)((int)e1p + c1) & 0xffffu;   /* int16 wrap-on-store */
                big |= abs(pl_sext16((int)n0[p])) > 8000;
                bigl |= abs(pl_sext16((int)n0[p])) > PL_E0_LEAD_MAX;
                n1[p] = (uint32_t)c2 & 0xffffu;
            }
            perr0[x] = make_uint2(n0[0] | (n0[1] << 16), n0[2] | (n0[3] << 16));
            perr1[x] = make_uint2(n1[0] | (n1[1] << 16), n1[2] | (n1[3] << 16));
        }
        }
        if (big) big_err = 1;
        if (bigl) big_lead = 1;
        for (int b = tid; b < PL_NSYM; b += PL_ENGINE_THREADS) Hc[b] = tbl[winner][b].x;
        if (tid == 0 && j.row_filters) j.row_filters[y] = (uint8_t)(0x08u << winner);   /* PNG_FILTER_* flags */
        if (tid == 0) j.row_ids[y] = (uint8_t)winner;
        if (tid == 0 && j.progress) __hip_atomic_store(j.progress, y + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        cyc_commit += __builtin_readcyclecounter() - tcm0;
        __syncthreads();
    }

    /* ---- epilogue: final histogram + result record (pngloss_image.c:311-325) ---- */
    uint32_t nz = 0;
    for (int b = tid; b < PL_NSYM; b += PL_ENGINE_THREADS) {
        j.final_hist[b] = Hc[b];
        nz += Hc[b] != 0;
    }
    if (tid == 0) uniq = 0;
    __syncthreads();
    if (nz) atomicAdd(&uniq, nz);
    __syncthreads();
    /* diagnostics: per chain wave, cycles spent in the serial chain (>>10) and pixels that needed the exact repair */
    if (lane == 0 && wave < PLR_WG_CHAIN_WAVES) {
        j.result[PLR_WG_CHAIN_KCYC + wave] = (int32_t)(chain_cycles >> 10);
        j.result[PLR_WG_SLOW_PX + wave] = (int32_t)slow_px;
    }
    if (lane == 0 && wave < PL_NFILT) {
        for (int qq = 0; qq < PLR_WG_PHASES; qq++) j.result[PLR_WG_PHASE_KCYC + wave * PLR_WG_PHASES + qq] = (int32_t)(lead_cyc[qq] >> 10);
        j.result[PLR_WG_CYC_PER_PX + wave] = (int32_t)(lead_cyc[PL_LC_CLEAN_PX] ? lead_cyc[PL_LC_CLEAN] / lead_cyc[PL_LC_CLEAN_PX] : 0);
        j.result[PLR_WG_FLUSH_KCYC + wave] = (int32_t)(lead_cyc[PL_LC_FLUSH] >> 10);   /* flush + relation check */
        j.result[PLR_WG_LIGHT_PX + wave] = (int32_t)light_px;
    }
    if (lane == 0 && wave == 0) { j.result[PLR_WG_POST_KCYC] = (int32_t)(cyc_post >> 10); j.result[PLR_WG_COMMIT_KCYC] = (int32_t)(cyc_commit >> 10); }
    {   /* diagnostics: which SIMD each wave of the workgroup sits on (HW_ID bits 5:4), two bits per wave */
        uint32_t hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        if (lane == 0) atomicOr(&simd_map, ((hwid >> 4) & 3u) << (2 * wave));
    }
    __syncthreads();
    if (tid == 0) j.result[PLR_WG_SIMD_MAP] = (int32_t)simd_map;
    if (tid == 0) { j.result[PLR_WG_EST_LEAD] = (int32_t)est_lead; j.result[PLR_WG_EST_LEGACY] = (int32_t)est_legacy; }
    if (tid == 0) j.result[PLR_WG_ADAPT_LEGACY] = (int32_t)adapt_legacy_rows;
    if (lane == 0 && wave == 4) {
        j.result[PLR_WG_W4_KCYC] = (int32_t)(chain_cycles >> 10);
        j.result[PLR_WG_W4_SLOW_PX] = (int32_t)slow_px;
        j.result[PLR_WG_W4_RESCANS] = (int32_t)lead_rebuilds;
    }
    if (tid == 0) {
        j.result[PLR_STATUS] = status;
        j.result[PLR_BPP] = (int32_t)bpp;
        j.result[PLR_UNIQUE] = (int32_t)uniq;
        j.result[PLR_RETRIED] = (int32_t)retried;
        j.result[PLR_REPAIRED] = (int32_t)slow_px;   /* wave 0's count of pixels that needed the exact channel repair / exact redo */
        j.result[PLR_WG_LEAD_ROWS] = (int32_t)lead_rows;
        j.result[PLR_WG_RESCANS] = (int32_t)lead_rebuilds;
    }
}

static_assert(PLR_WG_PHASES == PL_LC_BUILD + 1, "the phases that go out as PLR_WG_PHASE_KCYC: vector, fast groups, exact redo, rescan, table build");

int pl_engine_occupancy(void)
{
    int n = -1;
    if (hipFuncSetAttribute((const void *)pl_engine, hipFuncAttributeMaxDynamicSharedMemorySize, PL_WG_LAUNCH_BYTES) != hipSuccess) return -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pl_engine, PL_ENGINE_THREADS, PL_WG_LAUNCH_BYTES) != hipSuccess) return -1;
    return n;
}

hipError_t pl_launch_engine(const PlJob *d_jobs, const uint32_t *d_sel, size_t n, PlEngineParams prm, hipStream_t stream)
{
    if (!n) return hipSuccess;
    static std::atomic<unsigned> done{ 0 };
    const hipError_t e = pl_lds_optin((const void *)pl_engine, PL_WG_LAUNCH_BYTES, done);
    if (e != hipSuccess) {
        /* 104 KB of dynamic LDS per workgroup: a gfx950-class CU (160 KB) has it, the 64 KB parts do not */
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        fprintf(stderr, "pngloss_hip: the row engine needs %d bytes of LDS per workgroup (gfx950-class CU with 160 KB); device %d refused: %s\n",
                (int)PL_WG_LAUNCH_BYTES, dev, hipGetErrorString(e));
        return e;
    }
    hipLaunchKernelGGL(pl_engine, dim3((unsigned)n), dim3(PL_ENGINE_THREADS), PL_WG_LAUNCH_BYTES, stream, d_jobs, d_sel, prm);
    return hipGetLastError();
}

/*
 * pl_wg_chain.h -- workgroup engine (pl_engine.hip), part 2: the ROUND-1 CHAINS.  Lanes 16c..16c+15 = channel c of the current pixel (a DPP row) hold the
 * <= s+1 candidate symbols of that channel's band (optimize_state.c:186-214); per pixel: predict -> re-centre -> band -> clamp, gather of {running frequency,
 * rank of original frequency}, two DPP arg-max reductions of the reference's 4-level key, exact repair of the coupling between the channels of a pixel
 * (optimize_state.c:221,253).  They take the rows the band-leader chains (pl_wg_lead.h) cannot -- q > 128, exploding errors -- and the rows where those are
 * measurably slower.  Their LDS: the histogram tables and the split table of the fixed part, and a slot of chunk records per wave (pl_wg_lds.h, view
 * PL_WG_ROUND1).  A part of pl_engine.hip: included inside its anonymous namespace, behind pl_wg_util.h.
 */
#ifndef PL_WG_CHAIN_H
#define PL_WG_CHAIN_H

struct RowCtx {
    const uint32_t *row;      /* original row y (slots)                                  */
    const uint32_t *nabove;   /* optimised row y-1 or nullptr                            */
    const uint2 *err0;        /* incoming error for row y                                */
    uint4 *cand;              /* cand[5][W]: per candidate, per pixel: 4 x (byte | diff16<<8) */
    lds_uint2 *tbl;           /* tbl[5][PL_TBL_N] {H, rank<<9} in LDS                    */
    lds_uint4 *rec;           /* this WAVE's chunk records: [PL_CHUNK][4][1 or 2]         */
    lds_u32 *lut;             /* Sierra split table: [diff+256] -> rem | thr<<16, |diff|<=255 */
    uint32_t W, y, bpp;
    int s;
    float rq, rbleed, r29;
    uint32_t slow;            /* out: pixels that took the exact-repair slow path        */
    unsigned long long seg[4];/* out, always 0 and read by nobody: left from a removed timing experiment.  chain_dispatch is __noinline__
                                 and writes the RowCtx through a reference, so dropping the field and its stores changes the code object */
};

/* ---------------------------------------------------------------------------------------------------------
 * The serial chain of one wave over one row.
 *   MODE 1,3,4  one candidate filter (sub, average, paeth): 16 lanes per channel
 *   MODE 5      TWO candidate filters whose prediction does not depend on the left neighbour (none = half 0, up =
 *               half 1 of every 16-lane DPP row): 8 lanes per (channel, filter).  Five chains on four SIMDs would
 *               make two waves share a SIMD, and the younger of two DPP-heavy waves on one SIMD runs at half rate
 *               (profiles/r01_ubench_simd_sharing.txt) -- so the two cheapest chains share one wave instead.
 *   NCT  candidates per lane known at compile time (1..4) or 0 for the generic two-sweep loop
 *   TR   the image class has alpha (2 or 4 B/px): honour optimize_state.c:158-164 for fully transparent pixels
 *   WRAP false when every incoming error of this row is <= 8000 in magnitude (decided by the commit pass): then no
 *        intermediate can leave int16 (DESIGN.md "int16 wrap") and the sign-extensions are dropped
 * Per pixel (all channels at once): band -> candidates -> gather -> 2 DPP arg-max reductions, speculative w.r.t. the
 * histogram bumps of the earlier channels of the same pixel; a 1-pass test (one ds_bpermute) proves the speculation
 * harmless -- the common case -- or sends the pixel down the exact sequential repair.
 * --------------------------------------------------------------------------------------------------------- */
template <int MODE, int NCT, bool TR, bool WRAP>
__device__ __forceinline__ void chain_row(RowCtx &k, const int lane)
{
    constexpr bool PAIR = MODE == 5;
    constexpr int GL = PAIR ? 8 : 16;                     /* lanes per (channel[, filter]) group */
    const int c = lane >> 4, jl = lane & (GL - 1);
    const int half = PAIR ? (lane >> 3) & 1 : 0;
    const int filt_id = PAIR ? 2 * half : MODE;           /* which candidate filter this lane works for */
    const uint32_t bpp = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.bpp);
    const uint32_t W = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.W);
    glb_cu32 *const row = (glb_cu32 *)k.row, *const nabove = (glb_cu32 *)k.nabove;
    glb_cu32x2 *const err0 = (glb_cu32x2 *)k.err0;
    glb_u32 *const outp = (glb_u32 *)(k.cand + (size_t)filt_id * W);
    const bool active = (uint32_t)c < bpp;
    const int s = __builtin_amdgcn_readfirstlane(k.s), q = s + 1;
    const int nc = NCT ? NCT : (q + GL - 1) / GL;
    const float rq = k.rq, rbleed = k.rbleed, r29 = k.r29;
    lds_uint2 *const T = k.tbl + filt_id * PL_TBL_N;
    lds_uint4 *const R = k.rec;
    lds_u32 *const LUT = k.lut;
    /* lane constants */
    const bool upd = active && jl == 0;                 /* the one lane per group that bumps the histogram        */
    const uint32_t inc = upd ? 1u : 0u;
    const int dummy = PL_NSYM + lane;
    const bool chk = active && jl < c && jl < 3;        /* lane (c, k<c) checks channel k's bump against channel c */
    /* the same facts as sign/bit masks, so that the per-pixel test stays in the VALU: a VALU-written lane mask that
     * is read by the SALU costs ~16-28 cycles on gfx950 (profiles/r01_ubench_mask_traffic.txt) */
    const int nochk_neg = chk ? 0 : (int)0x80000000;    /* forces "no conflict" in lanes that do not check            */
    const int inact_neg = active ? 0 : (int)0x80000000; /* forces "in range" in lanes of unused channel rows          */
    const int upd_and = upd ? 255 : 0, upd_or = upd ? 0 : dummy;
    const bool sel0 = jl == 0, sel1 = jl == 1;          /* which earlier channel this lane checks                  */
    uint32_t slow = 0;

    int left = 0, rem = 0, thr_prev = 0, thr_cur = 0;

    constexpr int RS = PAIR ? 2 : 1;                    /* records per (pixel, channel) */
    for (uint32_t x0 = 0; x0 < W; x0 += PL_CHUNK) {
        /* ---- vector pre-phase: lane = pixel x0+lane; everything that does not depend on the chain ---- */
        bool chunk_has_transparent = false;
        if (lane < PL_CHUNK) {
            const uint32_t xl = x0 + lane;
            const bool ok = xl < W;
            const uint32_t o = ok ? row[xl] : 0u;
            const uint32_t a = (ok && nabove) ? nabove[xl] : 0u;
            const uint32_t d = (ok && nabove && xl) ? nabove[xl - 1] : 0u;
            const u32x2 e = ok ? err0[xl] : (u32x2){ 0u, 0u };
            const bool alpha0 = TR && (bpp & 1u) == 0u && ((o >> (8u * (bpp - 1u))) & 255u) == 0u;   /* only 2 and 4 B/px have alpha */
            chunk_has_transparent = alpha0;
#pragma unroll
            for (int cc = 0; cc < 4; cc++) {
                const int p = pl_plane_of_channel(bpp, cc);
                const int e0 = pl_sext16((int)(p < 2 ? (e.x >> (16 * p)) : (e.y >> (16 * (p - 2)))));
                const int orig = (o >> (8 * cc)) & 255, above = (a >> (8 * cc)) & 255, diag = (d >> (8 * cc)) & 255;
                const uint32_t trbit = (alpha0 && (uint32_t)cc == bpp - 1u) ? (1u << 16) : 0u;
                if (PAIR) {
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int pred = h ? above : 0;
                        const int osym = pl_sext8(orig - pred);
                        R[(lane * 4 + cc) * RS + h] = (u32x4){ (uint32_t)osym, (uint32_t)(osym - orig), (uint32_t)pred | trbit,
                                                              (uint32_t)(WRAP ? e0 : osym + e0) };
                    }
                } else {
                    R[(lane * 4 + cc) * RS] = (u32x4){ (uint32_t)orig, (uint32_t)above, (uint32_t)diag | trbit, (uint32_t)e0 };
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int n = (int)min((uint32_t)PL_CHUNK, W - x0);
        /* the serial part of the chunk, compiled twice: with and without the fully-transparent-pixel handling, chosen per
         * chunk (most chunks of most images have no alpha == 0 pixel, and the handling costs ~6 issue slots per pixel) */
        auto serial_part = [&](auto trx_tag) {
        constexpr bool TRX = decltype(trx_tag)::value;
        u32x4 r = R[c * RS + half];
        for (int g = 0; g < n; g += GL) {
        const int m = min(GL, n - g);
        /* one pixel step; called twice per loop iteration (manual 2x unroll: halves the loop-control and back-edge cost
         * and lets the record registers alternate instead of being copied) */
        auto pixel = [&](const int ii) {
            const int i = g + ii;
            const u32x4 rn = R[(((i + 1) & (PL_CHUNK - 1)) * 4 + c) * RS + half];   /* prefetch the next pixel's record */

            /* ---- uniform per group: optimize_state.c:157-210 ---- */
            int osym, lo, predraw, filt;
            if (PAIR) {
                osym = (int)r.x; lo = (int)r.y; predraw = (int)(r.z & 0xffffu);
                filt = WRAP ? osym + pl_sext16((int)r.w + rem + thr_prev) : (int)r.w + rem + thr_prev;
            } else {
                const int orig = (int)r.x;
                if (MODE == 4) {
                    /* Paeth with three v_sad_u32 (|a-b|+0) instead of sub/neg/max triplets */
                    const uint32_t ab = r.y, dg = r.z & 0xffffu, lf = (uint32_t)left;
                    const uint32_t dl = sad_u32(ab, dg), da = sad_u32(lf, dg), dd = sad_u32(lf + ab, dg + dg);
                    predraw = (dl <= da && dl <= dd) ? left : (da <= dd ? (int)ab : (int)dg);
                } else {
                    predraw = pl_predict<MODE>((int)r.y, (int)(r.z & 0xffffu), left);
                }
                osym = pl_sext8(orig - predraw);
                lo = osym - orig;                       /* = -(re-centred prediction), optimize_state.c:175-182 */
                int err = (int)r.w + rem + thr_prev;
                if (WRAP) err = pl_sext16(err);
                filt = osym + err;
            }
            const int tq = (int)((float)filt * rq);     /* trunc(filt / q), exact (pl_device.h) */
            int vmin = __mul24(tq, q) - ((filt >> 31) & s);
            int vmax = vmin + s;
            const int hi = lo + 255;
            vmin = med3_i32(vmin, lo, hi);
            vmax = med3_i32(vmax, lo, hi);
            bool tr = false;
            if (TRX) {
                tr = (r.z >> 16) != 0;                  /* optimize_state.c:158-164 */
                vmin = tr ? -predraw : vmin;
                vmax = tr ? -predraw : vmax;
                lo = tr ? -predraw : lo;
            }
            const int span = vmax - vmin, josym = osym - vmin;

            /* ---- candidates: gather and two-level arg-max (optimize_state.c:212-244).  Lanes beyond the band
             *      re-evaluate its last member, which cannot change a max or an arg-max. ---- */
            uint32_t Hwin, K;
            if (NCT) {
                int jj[NCT ? NCT : 1];
                u32x2 e[NCT ? NCT : 1];
                uint32_t kk[NCT ? NCT : 1];
#pragma unroll
                for (int t = 0; t < NCT; t++) {
                    jj[t] = min(jl + GL * t, span);
                    e[t] = T[(vmin + jj[t]) & 255];
                }
                uint32_t hm = e[0].x;
#pragma unroll
                for (int t = 0; t < NCT; t++) {
                    kk[t] = e[t].y + ((jj[t] == josym) ? 256u : 0u) + (uint32_t)(256 - jj[t]);
                    hm = max(hm, e[t].x);
                }
                Hwin = groupmax_u32<GL>(hm);
                uint32_t km = 0;
#pragma unroll
                for (int t = 0; t < NCT; t++) km = max(km, e[t].x == Hwin ? kk[t] : 0u);
                K = groupmax_u32<GL>(km);
            } else {
                uint32_t hm = 0;
                for (int t = 0; t < nc; t++) hm = max(hm, T[(vmin + min(jl + GL * t, span)) & 255].x);
                Hwin = groupmax_u32<GL>(hm);
                uint32_t km = 0;
                for (int t = 0; t < nc; t++) {
                    const int j2 = min(jl + GL * t, span);
                    const u32x2 e = T[(vmin + j2) & 255];
                    km = max(km, e.x == Hwin ? e.y + ((j2 == josym) ? 256u : 0u) + (uint32_t)(256 - j2) : 0u);
                }
                K = groupmax_u32<GL>(km);
            }
            int jwin = (int)((0u - K) & 255u);          /* K-1 = rank<<9 | flag<<8 | 255-j */
            int vwin = vmin + jwin;

            /* histogram bump, issued NOW with the speculative winner so that the LDS atomic retires behind the check
             * below instead of in front of the next pixel's record wait; the rare repair path moves it.  EXEC is not
             * touched: non-owner lanes add 0 to a private dummy slot. */
            const int bump_idx = (vwin & upd_and) | upd_or;
            __hip_atomic_fetch_add((lds_u32 *)&T[bump_idx], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);

            /* ---- did an earlier channel of this pixel bump a bin of my band that is not my winner?
             *      lane (c, k) looks at channel k's (speculative) winner: readlane broadcasts + lane-constant selects,
             *      no LDS round trip; the split-table read issued below overlaps with this arithmetic ---- */
            int sv;
            if (PAIR) {
                const int a0 = __builtin_amdgcn_readlane(vwin, 0), a1 = __builtin_amdgcn_readlane(vwin, 16), a2 = __builtin_amdgcn_readlane(vwin, 32);
                const int b0 = __builtin_amdgcn_readlane(vwin, 8), b1 = __builtin_amdgcn_readlane(vwin, 24), b2 = __builtin_amdgcn_readlane(vwin, 40);
                const int sa = sel0 ? a0 : (sel1 ? a1 : a2), sb = sel0 ? b0 : (sel1 ? b1 : b2);
                sv = half ? sb : sa;
            } else {
                const int a0 = __builtin_amdgcn_readlane(vwin, 0), a1 = __builtin_amdgcn_readlane(vwin, 16), a2 = __builtin_amdgcn_readlane(vwin, 32);
                sv = sel0 ? a0 : (sel1 ? a1 : a2);
            }

            /* ---- reconstruct (optimize_state.c:251-260); the Sierra terms that stay in this row (:455,467) come
             *      from a 511-entry LDS table of the split, fetched alongside the ds_bpermute above ---- */
            int back = vwin - lo;
            int diff = filt - vwin;
            if (WRAP) diff = pl_sext16(diff);
            if (TRX) diff = tr ? 0 : diff;
            uint32_t le = LUT[(diff + 256) & 511];
            int remv, thrv;
            int sv2 = sv;

            /* bad  <=>  (checking lane: channel k's winner lies in my band and is not my winner) or |diff| > 255.
             * z >= 0 <=> conflict, w >= 0 <=> table index out of range; one compare, one branch. */
            const int tt = (sv2 - vmin) & 255;
            const int z = ((tt != jwin) ? span - tt : -1) | nochk_neg;
            const int w = (max(diff, -diff) - 256) | inact_neg;
            const bool bad = (z & w) >= 0;
            /* consume the split-table entry HERE: otherwise the compiler sinks its ds_read below the branch, where the
             * whole LDS latency lands on the critical path; issued ~15 slots ago it has (nearly) arrived by now */
            asm volatile("" : "+v"(le));
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
                /* exact repair in channel order: channel cp chose bin sb and bumped it to sH */
                slow++;
                uint32_t Rwin = (K - 1u) >> 9;
#pragma unroll
                for (int cp = 0; cp < 3; cp++) {
                    if ((uint32_t)cp + 1u < bpp) {
                        int sb; uint32_t sH, sR;
                        if (PAIR) {
                            const int b0 = __builtin_amdgcn_readlane(vwin, 16 * cp), b1 = __builtin_amdgcn_readlane(vwin, 16 * cp + 8);
                            const int h0 = __builtin_amdgcn_readlane((int)Hwin, 16 * cp), h1 = __builtin_amdgcn_readlane((int)Hwin, 16 * cp + 8);
                            const int r0 = __builtin_amdgcn_readlane((int)Rwin, 16 * cp), r1 = __builtin_amdgcn_readlane((int)Rwin, 16 * cp + 8);
                            sb = half ? b1 : b0; sH = (uint32_t)(half ? h1 : h0) + 1u; sR = (uint32_t)(half ? r1 : r0);
                        } else {
                            sb = __builtin_amdgcn_readlane(vwin, 16 * cp);
                            sH = (uint32_t)__builtin_amdgcn_readlane((int)Hwin, 16 * cp) + 1u;
                            sR = (uint32_t)__builtin_amdgcn_readlane((int)Rwin, 16 * cp);
                        }
                        const int jj2 = (sb - vmin) & 255;
                        const uint32_t K2 = (sR << 9) + ((jj2 == josym) ? 256u : 0u) + (uint32_t)(256 - jj2);
                        const bool better = (c > cp) & (jj2 <= span) & ((sH > Hwin) | ((sH == Hwin) & (K2 > K)));
                        Hwin = better ? sH : Hwin;
                        K = better ? K2 : K;
                        jwin = better ? jj2 : jwin;
                        Rwin = better ? sR : Rwin;
                        vwin = vmin + jwin;
                    }
                }
                /* move the speculative bump to the repaired winner (no-op where nothing changed) */
                __hip_atomic_fetch_add((lds_u32 *)&T[bump_idx], 0u - inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add((lds_u32 *)&T[(vwin & upd_and) | upd_or], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                back = vwin - lo;
                diff = filt - vwin;
                if (WRAP) diff = pl_sext16(diff);
                if (TRX) diff = tr ? 0 : diff;
                const PlSplit sp = pl_sierra_split(diff, rbleed, r29);
                remv = (int)sp.rem;
                thrv = (int)sp.h;
            } else {
                remv = pl_sext16((int)le);
                thrv = (int)le >> 16;
            }
            thr_prev = thr_cur;
            thr_cur = thrv;
            rem = remv;
            left = back;
            /* output capture: the pixel's record is dead once `r` holds it, so its first word takes the result (one
             * ds_write, all lanes of the group the same word); lane jl picks up pixel g+jl when the group is done */
            const uint32_t packed = (uint32_t)back | ((uint32_t)diff << 8);
            *(lds_u32 *)&R[((i & (PL_CHUNK - 1)) * 4 + c) * RS + half] = packed;
            r = rn;
        };
        int ii = 0;
        for (; ii + 1 < m; ii += 2) { pixel(ii); pixel(ii + 1); }
        if (ii < m) pixel(ii);
        if (active && jl < m) outp[(size_t)(x0 + g + jl) * 4 + c] = *(lds_u32 *)&R[(((g + jl) & (PL_CHUNK - 1)) * 4 + c) * RS + half];
        }
        };
        if (TR && __builtin_amdgcn_ballot_w64(chunk_has_transparent) != 0) serial_part(std::true_type{});
        else serial_part(std::false_type{});
    }
    k.slow = slow;
    k.seg[0] = 0; k.seg[1] = 0; k.seg[2] = 0; k.seg[3] = 0;
}

template <int MODE, bool TR, bool WRAP>
__device__ __forceinline__ void chain_dispatch_nc(RowCtx &k, int lane)
{
    const int q = k.s + 1;
    const int per_lane = (q + (MODE == 5 ? 7 : 15)) / (MODE == 5 ? 8 : 16);
    switch (per_lane) {
    case 1: chain_row<MODE, 1, TR, WRAP>(k, lane); break;   /* s <= 15 (paired wave: s <= 7)  */
    case 2: chain_row<MODE, 2, TR, WRAP>(k, lane); break;   /* s <= 31 (<= 15)                */
    case 3: chain_row<MODE, 3, TR, WRAP>(k, lane); break;   /* s <= 47 (<= 23): the default s=19 pairs here */
    case 4: chain_row<MODE, 4, TR, WRAP>(k, lane); break;   /* s <= 63 (<= 31)                */
    case 5: chain_row<MODE, 5, TR, WRAP>(k, lane); break;
    case 6: chain_row<MODE, 6, TR, WRAP>(k, lane); break;   /* s <= 95 (<= 47)                */
    default: chain_row<MODE, 0, TR, WRAP>(k, lane); break;  /* generic two-sweep loop         */
    }
}

template <int MODE>
__device__ __noinline__ void chain_dispatch(RowCtx &k, int lane, bool wrap)
{
    const bool tr = (k.bpp & 1u) == 0;
    if (wrap) {
        /* rare (needs |error| > 8000): one careful variant is enough */
        chain_row<MODE, 0, true, true>(k, lane);
    } else if (tr) chain_dispatch_nc<MODE, true, false>(k, lane);
    else chain_dispatch_nc<MODE, false, false>(k, lane);
}

#endif

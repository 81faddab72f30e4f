/*
 * pl_wg_post.h -- workgroup engine (pl_engine.hip), part 4: the POST PASS of a row attempt's candidates, parallel over x.  A part of pl_engine.hip: included
 * inside its anonymous namespace, behind pl_wg_util.h.
 */
#ifndef PL_WG_POST_H
#define PL_WG_POST_H

/* ---------------------------------------------------------------------------------------------------------
 * Per-candidate post pass, parallel over x (lane = pixel): derivative error (optimize_state.c:265-287),
 * libpng's heuristic filter (optimize_state.c:492-562) and entropy cost (optimize_state.c:326-342).
 * Returns the row cost of optimize_state_row (optimize_state.c:360) or UINT64_MAX if rejected (:319-324).
 * --------------------------------------------------------------------------------------------------------- */
/* All five candidates at once, parallel over x with every thread of the workgroup: the neighbourhood of a pixel (original
 * and optimised rows) is loaded once for the five candidates; per-wave partial sums go to the LDS accumulators
 * acc[f] = { derr (u64 as two u32 adds: low, high), cost, hs[5] } (PL_PA_* of pl_wg_lds.h: PL_PA_WORDS per candidate, zeroed by the caller). */
/* (first, stride): the pixels this thread takes -- (tid, workgroup size) for the joint pass, (lane, 64) when one wave does a
 * candidate of its own while the other chains still run; fmask: the candidates to do */
__device__ void post_pass_all(const PlJob &j, uint32_t y, uint32_t bpp, const uint2 (*tbl)[PL_TBL_N], bool adaptive, int tid, uint32_t *acc,
                              uint32_t first, uint32_t stride, uint32_t fmask)
{
    const uint32_t W = j.width;
    const uint32_t *row = j.img + (size_t)y * W;
    const uint32_t *nab = y ? row - W : nullptr;
    uint64_t derr[PL_NFILT] = { 0, 0, 0, 0, 0 };
    uint32_t cost[PL_NFILT] = { 0, 0, 0, 0, 0 };
    uint32_t hs[PL_NFILT][PL_NFILT] = { { 0 } };
    for (uint32_t x = first; x < W; x += stride) {
        const uint32_t o = row[x], ol = x ? row[x - 1] : 0u;
        const uint32_t na = nab ? nab[x] : 0u, nd = (nab && x) ? nab[x - 1] : 0u;
        const uint32_t oa = y ? j.old_above[x] : 0u, od = (y && x) ? j.old_above[x - 1] : 0u;
#pragma unroll
        for (int f = 0; f < PL_NFILT; f++) {
            if (!((fmask >> f) & 1u)) continue;
            const uint4 cw = j.cand[(size_t)f * W + x];
            const uint4 cl = x ? j.cand[(size_t)f * W + x - 1] : make_uint4(0, 0, 0, 0);
            const uint32_t cws[4] = { cw.x, cw.y, cw.z, cw.w }, cls[4] = { cl.x, cl.y, cl.z, cl.w };
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if ((uint32_t)c < bpp) {
                    const int sh = 8 * c;
                    const int back = cws[c] & 255, nl = x ? (int)(cls[c] & 255) : 0;
                    const int ov = (o >> sh) & 255, olv = (ol >> sh) & 255;
                    const int nav = (na >> sh) & 255, ndv = (nd >> sh) & 255, oav = (oa >> sh) & 255, odv = (od >> sh) & 255;
                    const int da = (oav - ov) - (nav - back);
                    const int dd = (odv - ov) - (ndv - back);
                    const int dl = (olv - ov) - (nl - back);
                    const uint32_t w = (bpp <= 2 && c == 0) ? 3u : 1u;      /* gray is replicated into r,g,b (color_delta.c:11-26) */
                    derr[f] += (uint64_t)(w * (uint32_t)(da * da + dd * dd + dl * dl));
                    const int pred = f == 0 ? 0 : (f == 1 ? nl : (f == 2 ? nav : (f == 3 ? (nav + nl) >> 1 : pl_paeth(nav, ndv, nl))));
                    cost[f] += 33u + (uint32_t)__clz((int)tbl[f][(back - pred) & 255].x);
                    if (adaptive) {
                        const int preds[PL_NFILT] = { 0, nl, nav, (nav + nl) >> 1, pl_paeth(nav, ndv, nl) };
#pragma unroll
                        for (int g = 0; g < PL_NFILT; g++) {
                            const int bb = (back - preds[g]) & 255;
                            hs[f][g] += (uint32_t)(bb < 128 ? bb : 256 - bb);
                        }
                    }
                }
            }
        }
    }
    const int lane = tid & 63;
#pragma unroll
    for (int f = 0; f < PL_NFILT; f++) {
        if (!((fmask >> f) & 1u)) continue;
        const uint64_t d = wave_sum_u64(derr[f]);
        const uint32_t cs = wave_sum_u32(cost[f]);
        if (lane == 0) {
            atomicAdd((unsigned long long *)&acc[PL_PA_WORDS * f + PL_PA_DERR], (unsigned long long)d);
            atomicAdd(&acc[PL_PA_WORDS * f + PL_PA_COST], cs);
        }
        if (adaptive) {
#pragma unroll
            for (int g = 0; g < PL_NFILT; g++) {
                const uint32_t v = wave_sum_u32(hs[f][g]);
                if (lane == 0) atomicAdd(&acc[PL_PA_WORDS * f + PL_PA_HS + g], v);
            }
        }
    }
}

#endif

/*
 * pl_prepost_core.h -- the rules of the streaming kernels around the row engine (pl_prepost.hip), stated once for the device and for the CPU:
 *
 *   pl_sub4 / pl_avg4        byte-wise arithmetic on the four channel bytes of a pixel word, no carry across bytes
 *   plp_bins                 the five bins (one per PNG predictor) that one channel of one pixel adds to original_frequency
 *                            (optimize_state.c:66-83: (byte - prediction) mod 256, predictions from the ORIGINAL neighbours)
 *   plp_quad_loader          which of pl_hist's two loaders an image gets
 *   plp_quad_at / plp_pixel_at   where a step of either loader finds its neighbours
 *   plp_hist_thread          the share of one thread of pl_hist: its steps at the stride of the image's workgroups, through either loader
 *   plp_rank                 the 8-bit rank pl_rank stores for a bin
 *   plp_batch_blocks, plp_hist_blocks, PLP_MAX_IMAGES   the launch shapes
 *
 * Shared by pl_prepost.hip (pl_rows.hip and pl_emit.hip take PLP_MAX_IMAGES) and by tests/c/prepost_host.cpp (test infrastructure), which runs the
 * same thread loop for every (workgroup, thread) of a launch on the CPU under the sanitizers.
 */
#ifndef PL_PREPOST_CORE_H
#define PL_PREPOST_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLP_HD __host__ __device__ __forceinline__
#else
#define PLP_HD inline
#endif

constexpr int PLP_NFILT = 5, PLP_NSYM = 256;

/* ---- byte-wise arithmetic in one word ---- */
PLP_HD uint32_t pl_sub4(uint32_t a, uint32_t b)      /* per byte (a - b) mod 256 */
{
    return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ (~(a ^ b) & 0x80808080u);
}
PLP_HD uint32_t pl_avg4(uint32_t a, uint32_t b)      /* per byte floor((a + b) / 2) */
{
    return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1);
}

/* the Paeth predictor (optimize_state.c:575-613; pl_device.h:pl_paeth is the same rule for the engines).  All operands 0..255. */
PLP_HD int plp_paeth(int above, int diag, int left)
{
    const int p = above - diag, pd = left - diag;
    const int pl = p < 0 ? -p : p, pa = pd < 0 ? -pd : pd, pg = p + pd < 0 ? -(p + pd) : p + pd;
    return (pl <= pa && pl <= pg) ? left : (pa <= pg ? above : diag);
}

/* the residual words of a pixel under sub, up and average: all four channel bytes at once */
struct PlpResidual { uint32_t sub, up, avg; };
PLP_HD PlpResidual plp_residual(uint32_t here, uint32_t left, uint32_t above)
{
    return PlpResidual{ pl_sub4(here, left), pl_sub4(here, above), pl_sub4(here, pl_avg4(above, left)) };
}

/* bin[f] of channel c (byte c of the words): none, sub, up, average, paeth */
PLP_HD void plp_bins(uint32_t bin[PLP_NFILT], int c, uint32_t here, uint32_t left, uint32_t above, uint32_t diag, const PlpResidual &r)
{
    const int hv = (here >> (8 * c)) & 255, lv = (left >> (8 * c)) & 255;
    const int av = (above >> (8 * c)) & 255, dv = (diag >> (8 * c)) & 255;
    bin[0] = (uint32_t)hv;
    bin[1] = (r.sub >> (8 * c)) & 255u;
    bin[2] = (r.up >> (8 * c)) & 255u;
    bin[3] = (r.avg >> (8 * c)) & 255u;
    bin[4] = (uint32_t)((hv - plp_paeth(av, dv, lv)) & 255);
}

/* ---- the two loaders of pl_hist ----
 * The quad loader takes four neighbouring pixels a step (one 16-byte load per row, left / diagonal neighbours of the last three from registers).
 * It needs rows that are a whole number of quads -- a quad then never straddles two rows --, an image that starts on 16 bytes, and a pixel count
 * whose quad index fits 32 bits.  Every other image goes pixel by pixel. */
struct alignas(16) PlpQuad { uint32_t x, y, z, w; };

PLP_HD bool plp_quad_loader(uint32_t W, const void *img, size_t n)
{
    return !(W & 3u) && !(reinterpret_cast<uintptr_t>(img) & 15u) && n < 0xffffffffull;
}

/* quad q of an image of W4 quads a row: is there a row above, a pixel to the left; the quad above, the pixels left of the quad and of the one above */
struct PlpQuadAt { bool has_up, has_left; uint32_t up; size_t left, diag; };
PLP_HD PlpQuadAt plp_quad_at(uint32_t q, uint32_t W4)
{
    PlpQuadAt a;
    a.has_up = q >= W4;
    a.has_left = (q % W4) != 0u;
    a.up = a.has_up ? q - W4 : 0u;
    a.left = a.has_left ? (size_t)q * 4 - 1 : 0;
    a.diag = (a.has_up && a.has_left) ? (size_t)(q - W4) * 4 - 1 : 0;
    return a;
}

/* pixel i of an image W pixels wide, the same questions */
struct PlpPixelAt { bool has_up, has_left; size_t up, left, diag; };
PLP_HD PlpPixelAt plp_pixel_at(size_t i, uint32_t W)
{
    PlpPixelAt a;
    a.has_up = i >= W;
    a.has_left = (uint32_t)(i % W) != 0u;
    a.up = a.has_up ? i - W : 0;
    a.left = a.has_left ? i - 1 : 0;
    a.diag = (a.has_up && a.has_left) ? i - W - 1 : 0;
    return a;
}

/* The share of thread `thread` of workgroup `block`, of `blocks` workgroups of NT threads each: steps block * NT + thread, + blocks * NT, ...
 * count(here, left, above, diag) is called once per pixel with the pixel's word and its three neighbours' (0 where the image has none). */
template <class Count>
PLP_HD void plp_hist_thread(const uint32_t *__restrict__ img, uint32_t W, size_t n, uint32_t block, uint32_t thread, uint32_t blocks, uint32_t NT, Count &&count)
{
    if (plp_quad_loader(W, img, n)) {
        const PlpQuad *__restrict__ img4 = reinterpret_cast<const PlpQuad *>(img);
        const uint32_t W4 = W >> 2, nq = (uint32_t)(n >> 2);
        for (uint32_t q = block * NT + thread; q < nq; q += blocks * NT) {
            const PlpQuadAt at = plp_quad_at(q, W4);
            const PlpQuad hq = img4[q];
            PlpQuad aq = { 0u, 0u, 0u, 0u };
            uint32_t left = 0u, diag = 0u;
            if (at.has_up) aq = img4[at.up];
            if (at.has_left) left = img[at.left];
            if (at.has_up && at.has_left) diag = img[at.diag];
            count(hq.x, left, aq.x, diag);
            count(hq.y, hq.x, aq.y, aq.x);
            count(hq.z, hq.y, aq.z, aq.y);
            count(hq.w, hq.z, aq.w, aq.z);
        }
    } else {
        for (size_t i = (size_t)block * NT + thread; i < n; i += (size_t)blocks * NT) {
            const PlpPixelAt at = plp_pixel_at(i, W);
            const uint32_t here = img[i];
            const uint32_t left = at.has_left ? img[at.left] : 0u;
            const uint32_t above = at.has_up ? img[at.up] : 0u;
            const uint32_t diag = (at.has_up && at.has_left) ? img[at.diag] : 0u;
            count(here, left, above, diag);
        }
    }
}

/* ---- pl_rank: rank of a bin that counted `mine` = #{ b' : h[b'] < mine } over the 256 bins of its table (0..255): a < b <=> rank(a) < rank(b), and
 * a == b <=> rank(a) == rank(b), which is all optimize_state.c:228-235 uses the secondary key for ---- */
PLP_HD uint32_t plp_rank(const uint32_t *h, uint32_t mine)
{
    uint32_t r = 0;
    for (int k = 0; k < PLP_NSYM; k++) r += h[k] < mine;
    return r;
}

/* ---- the launch shapes.  blockIdx.y = image: a launch takes at most PLP_MAX_IMAGES images (gridDim.y), a larger batch goes in slices, each launch
 * starting at its own jobs.  Per image (blockIdx.x) a slice of n images whose largest has max_px pixels gets
 *   plp_batch_blocks  (pl_classify, pl_repack, pl_unpack: 256 threads, px_per_thread pixels a thread) min(needed, max(8, ceil(2048 / n))) workgroups,
 *   plp_hist_blocks   (pl_hist: NT threads, 16 pixels a thread) min(needed, max(4, ceil(wgs_cap / n))) workgroups,
 * at least one: enough to fill 256 CUs several times over, never more than the batch needs.  n >= 1. ---- */
constexpr size_t PLP_MAX_IMAGES = 65535;
constexpr uint32_t PLP_THREADS = 256;

inline size_t plp_batch_blocks(size_t n, size_t max_px, uint32_t px_per_thread)
{
    if (max_px < 1) max_px = 1;
    size_t blocks = (max_px + (size_t)PLP_THREADS * px_per_thread - 1) / ((size_t)PLP_THREADS * px_per_thread);
    size_t cap = (2048 + n - 1) / n;
    if (cap < 8) cap = 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

inline size_t plp_hist_blocks(size_t n, size_t max_px, uint32_t NT, unsigned wgs_cap)
{
    if (max_px < 1) max_px = 1;
    size_t blocks = (max_px + (size_t)NT * 16 - 1) / ((size_t)NT * 16);
    size_t cap = (wgs_cap + n - 1) / n;
    if (cap < 4) cap = 4;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

/* the slice of a batch of n images that starts at image `first` */
inline size_t plp_slice(size_t n, size_t first) { return n - first < PLP_MAX_IMAGES ? n - first : PLP_MAX_IMAGES; }

#endif

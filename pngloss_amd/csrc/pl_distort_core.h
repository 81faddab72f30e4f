/*
 * pl_distort_core.h -- the arithmetic of the distortion measurement: how far the optimised RGBA8 image is from the original one.  No reference
 * equivalent (the reference tool reports file sizes only).  Per image, over its pixel pairs (a = original, b = optimised; little-endian words,
 * R in the low byte, channel c in byte c):
 *     sq_err[c]       sum of (b_c - a_c)^2, exact in 64 bits
 *     max_abs[c]      max of |b_c - a_c|
 *     changed_pixels  pixels whose words differ
 *     pixels          width * height
 * Everything is an integer, so the record does not depend on the order the pixels are summed in: the kernel's thousands of lanes and a loop on the
 * CPU give the same 64 bytes.
 * In visible mode (pld_thread<true>; below) the same sums are taken on alpha-premultiplied pixels and `pixels` counts the visible ones.
 *
 * Shared by the HIP kernel (pl_distort.hip: one thread runs pld_thread, the sums of the threads are merged through the wave, the workgroup and one
 * atomic per quantity) and by tests/c/distort_host.cpp and tests/c/visible_host.cpp (test infrastructure), which run the same thread loop on the CPU
 * under the sanitizers.
 */
#ifndef PL_DISTORT_CORE_H
#define PL_DISTORT_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLD_HD __host__ __device__ __forceinline__
#else
#define PLD_HD inline
#endif

/* the record of one image as the kernel writes it: the layout of pngloss_hip_distortion (include/pngloss_hip.h; pl_host_ctx.h asserts it) */
struct PlDistortRecord {
    uint64_t pixels, changed_pixels;
    uint64_t sq_err[4];
    uint32_t max_abs[4];
};
static_assert(sizeof(PlDistortRecord) == 64, "PlDistortRecord: six 64-bit words and four 32-bit ones, no padding");

/* A lane keeps its partial sums in 32 bits: one channel error is at most 255^2, so a 32-bit sum holds PLD_LANE_PIXELS_MAX (66 051) of them.  It is
 * emptied into the 64-bit sums once it has taken PLD_FLUSH_PIXELS pixels; a step of the vector loop adds four pixels, so a lane never holds more
 * than PLD_FLUSH_PIXELS + 3. */
constexpr uint32_t PLD_CHANNEL_SQ_MAX = 255u * 255u;
constexpr uint32_t PLD_LANE_PIXELS_MAX = 0xFFFFFFFFu / PLD_CHANNEL_SQ_MAX;
constexpr uint32_t PLD_FLUSH_PIXELS = 16384;
static_assert(PLD_FLUSH_PIXELS + 3 <= PLD_LANE_PIXELS_MAX, "a lane's 32-bit sums would overflow before they are flushed");

struct PldLane { uint32_t sq[4], mx[4], changed, visible; };          /* of at most PLD_FLUSH_PIXELS + 3 pixels */
struct PldSum { uint64_t sq[4], changed; uint32_t mx[4]; uint64_t visible; };  /* of any number of pixels (visible: counted in visible mode only) */

/* four pixels behind one 16-byte load */
struct alignas(16) PldQuad { uint32_t px[4]; };

/* ---- visible mode (include/pngloss_hip.h, "Measuring over visible pixels"): the same sums over the alpha-premultiplied pixels pm(a), pm(b), and
 * two counts that need the alpha of both: a pixel is visible when its alpha is non-zero in a or in b.  pm keeps alpha and turns each of R, G, B
 * into the integer nearest to c * A / 255 (255 is odd: no ties), at most 255 -- so every bound above holds as it stands.  An invisible pixel is
 * the word 0 in both images once premultiplied and adds nothing to any sum. ---- */
PLD_HD uint32_t pld_pm(uint32_t p)
{
    const uint32_t A = p >> 24;
    return ((( p        & 255u) * A + 127u) / 255u) | ((((p >> 8) & 255u) * A + 127u) / 255u) << 8 | ((((p >> 16) & 255u) * A + 127u) / 255u) << 16 |
           (p & 0xFF000000u);
}

template <bool Visible = false>
PLD_HD void pld_pixel(PldLane &l, uint32_t a, uint32_t b)
{
    if (Visible) {
        l.visible += ((a | b) >> 24) ? 1u : 0u;
        a = pld_pm(a);
        b = pld_pm(b);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 4; c++) {
        const int d = (int)((b >> (8 * c)) & 255u) - (int)((a >> (8 * c)) & 255u);
        const uint32_t m = (uint32_t)(d < 0 ? -d : d);
        l.sq[c] += m * m;
        l.mx[c] = m > l.mx[c] ? m : l.mx[c];
    }
    l.changed += a != b ? 1u : 0u;
}

PLD_HD void pld_flush(PldSum &s, PldLane &l)
{
    for (int c = 0; c < 4; c++) {
        s.sq[c] += l.sq[c];
        s.mx[c] = l.mx[c] > s.mx[c] ? l.mx[c] : s.mx[c];
        l.sq[c] = 0;
    }
    s.changed += l.changed;
    s.visible += l.visible;
    l.changed = l.visible = 0;
}

PLD_HD void pld_merge(PldSum &s, const PldSum &o)
{
    for (int c = 0; c < 4; c++) {
        s.sq[c] += o.sq[c];
        s.mx[c] = o.mx[c] > s.mx[c] ? o.mx[c] : s.mx[c];
    }
    s.changed += o.changed;
    s.visible += o.visible;
}

/* how many leading groups of four pixels go through 16-byte loads: all of them when both images start on a 16-byte boundary, else none
 * (the rest -- the n % 4 pixels of the tail, or the whole of a misaligned pair -- is taken word by word, as pl_classify does) */
PLD_HD size_t pld_vector_quads(const void *a, const void *b, size_t n)
{
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) ? 0 : n / 4;
}

/* the share of thread `tid` of `nthreads`: quads tid, tid + nthreads, ... of the vector part, then words at the same stride of the rest.
 * Visible: the visible mode above (the sums on premultiplied pixels, s.visible counted); without it s.visible stays 0 and is never read. */
template <bool Visible = false>
PLD_HD PldSum pld_thread(const uint32_t *a, const uint32_t *b, size_t n, size_t tid, size_t nthreads)
{
    PldSum s = {};
    PldLane l = {};
    uint32_t held = 0;
    const size_t n4 = pld_vector_quads(a, b, n);
    const PldQuad *a4 = reinterpret_cast<const PldQuad *>(a), *b4 = reinterpret_cast<const PldQuad *>(b);
    for (size_t i = tid; i < n4; i += nthreads) {
        const PldQuad va = a4[i], vb = b4[i];
        pld_pixel<Visible>(l, va.px[0], vb.px[0]);
        pld_pixel<Visible>(l, va.px[1], vb.px[1]);
        pld_pixel<Visible>(l, va.px[2], vb.px[2]);
        pld_pixel<Visible>(l, va.px[3], vb.px[3]);
        held += 4;
        if (held >= PLD_FLUSH_PIXELS) { pld_flush(s, l); held = 0; }
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nthreads) {
        pld_pixel<Visible>(l, a[i], b[i]);
        if (++held >= PLD_FLUSH_PIXELS) { pld_flush(s, l); held = 0; }
    }
    pld_flush(s, l);
    return s;
}

/* ---- the launch shape of pl_keep and pl_distort (pl_distort.hip), stated here so that a CPU test can pin it: PLD_THREADS lanes per workgroup, a
 * launch of at most PLD_MAX_IMAGES images (gridDim.y; a larger batch is launched in slices), and per image enough workgroups to give a lane 16 pixels
 * of the largest image, but only as many as fill 256 CUs several times over across the batch: min(needed, max(8, ceil(2048 / n))), at least 1.
 * A batch of 256 or more images so gets 8 workgroups -- 2048 lanes -- per image, however large its images are. ---- */
constexpr uint32_t PLD_THREADS = 256;
constexpr size_t PLD_MAX_IMAGES = 65535;

inline size_t pld_grid_blocks(size_t n, uint64_t max_pixels)
{
    size_t blocks = (size_t)((max_pixels + (uint64_t)PLD_THREADS * 16 - 1) / ((uint64_t)PLD_THREADS * 16));
    size_t cap = (2048 + n - 1) / n;
    if (cap < 8) cap = 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

/* the sums of all threads of an image, and its pixel count (visible mode: s.visible), as its record */
PLD_HD void pld_record(PlDistortRecord &r, const PldSum &s, uint64_t pixels)
{
    r.pixels = pixels;
    r.changed_pixels = s.changed;
    for (int c = 0; c < 4; c++) { r.sq_err[c] = s.sq[c]; r.max_abs[c] = s.mx[c]; }
}

/* Peak signal-to-noise ratio in dB of a record over the channels of `channel_mask` (bit c = channel c): the one formula behind pngloss_hip_psnr_db
 * (include/pngloss_hip.h says what it returns when) and behind the acceptance rule of pl_target.h.  Host arithmetic only. */
inline double pld_psnr_db(uint64_t pixels, const uint64_t sq_err[4], unsigned channel_mask)
{
    if (!pixels || !channel_mask || channel_mask > 0xFu) return (double)NAN;
    uint64_t sum = 0;
    int channels = 0;
    for (int c = 0; c < 4; c++)
        if (channel_mask & (1u << c)) { sum += sq_err[c]; channels++; }
    if (!sum) return (double)INFINITY;
    return 10.0 * log10(255.0 * 255.0 * (double)pixels * (double)channels / (double)sum);
}

#endif

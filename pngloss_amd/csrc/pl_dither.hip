/*
 * pl_dither.hip -- Floyd-Steinberg error diffusion on the device (gfx950; include/pngloss_hip_dither.h): the quantiser's remap step when dithering
 * is asked for.  The rule and the schedule are pl_dither_core.h's.
 *
 *   pl_dither   one workgroup per working image (blockIdx.x), one lane per row of a band of PLF_BAND rows, the waves PLF_LAG epochs apart, one
 *               barrier per epoch and no wait on memory anywhere.  The palette and its bases in LDS as in pl_quant_assign (every lane reads the
 *               same entry: a broadcast); per pixel the gather of the four errors, one search over the entries (plq_search<1>), one 4-byte store.
 *               A lane's errors stay in registers; the lane below takes the newest with a cross-lane move; lane 63 hands its errors to the
 *               next wave through a ring in LDS and, in the last wave, to the next band through the image's error line (plain vector stores and
 *               loads, a barrier between write and read).  A lane's pixels are loaded kAhead steps before their turn.
 *
 *   pl_dither_visible   the rule of the premultiplied space (include/pngloss_hip_quant_space.h): plf_pixel premultiplies the pixel, a pixel
 *               with alpha 0 takes no error in, and the word stored is the straight one of the nearest entry, from a second LDS table (1 KiB;
 *               lane e makes entry e's word at the kernel's start)
 *
 * A single image runs on one CU.  No kernel waits for another workgroup.  No reference equivalent.
 */
#include "pl_dither.h"

namespace {

constexpr int kThreads = (int)PLF_BAND;
constexpr uint32_t kAhead = 4;                  /* steps a pixel is loaded before the lane needs it: one register each */
static_assert(PLF_K % kAhead == 0, "the registers of the pixels in flight rotate a whole number of times per epoch");
static_assert(kThreads <= 1024 && kThreads % 64 == 0, "whole waves, one workgroup");

/* the premultiplied space keeps the straight word of every entry; pl_dither has no such table */
template <bool On>
__device__ __forceinline__ uint32_t *straight_table()
{
    if constexpr (On) {
        __shared__ uint32_t straight[PLQ_MAX_COLORS];
        return straight;
    } else {
        return nullptr;
    }
}

template <bool Visible>
__device__ __forceinline__ void dither_body(const PlDitherJob *__restrict__ jobs)
{
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    __shared__ PlfErr ring[PLF_RING_ENTRIES];
    uint32_t *const straight = straight_table<Visible>();
    const PlDitherJob j = jobs[blockIdx.x];
    const uint32_t W = j.width, H = j.height;
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    for (uint32_t e = threadIdx.x; e < entries; e += kThreads) {
        const uint32_t word = j.pal[e];
        pal2[2 * e] = word;
        pal2[2 * e + 1] = plq_base(word, e);
        if (Visible) straight[e] = plq_straight(word);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & (PLF_LANES - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / PLF_LANES);
    const uint64_t wave_epochs = plf_wave_epochs(W);
    const uint32_t bands = plf_bands(H);
    const PlfErr zero = { 0u, 0u };
    for (uint32_t band = 0; band < bands; band++) {
        const uint32_t rows = plf_band_rows(H, band), waves = plf_band_waves(rows);
        const uint64_t epochs = plf_band_epochs(W, waves);
        const uint32_t row = wave * PLF_LANES + lane;
        const bool has_row = row < rows;
        const size_t row_at = has_row ? ((size_t)band * PLF_BAND + row) * W : 0;
        const uint32_t *const src = j.img + row_at;
        uint32_t *const dst = j.out + row_at;
        const bool from_ring = wave > 0, from_line = wave == 0 && band > 0;
        const bool to_ring = wave + 1 < PLF_WAVES, to_line = !to_ring && band + 1 < bands;
        /* the error of column c of the row above lane 0's (c < W: the wave above, or the band above, has left it there) */
        auto above = [&](uint64_t c) -> PlfErr {
            if (c >= W) return zero;
            if (from_ring) return ring[plf_ring_index(wave, c)];
            if (from_line) return j.line[c];
            return zero;
        };
        auto pixel_at = [&](int64_t x) -> uint32_t { return has_row && x >= 0 && (uint64_t)x < W ? src[x] : 0u; };
        PlfLane s = { zero, zero, zero, zero };
        uint32_t q[kAhead] = {};
        for (uint64_t g = 0; g < epochs; g++) {
            const int64_t le = plf_local_epoch(g, wave);
            if (wave < waves && le >= 0 && (uint64_t)le < wave_epochs) {
                uint64_t t = (uint64_t)le * PLF_K;
                if (le == 0) {
                    if (lane == 0) s.ur = above(0);
#pragma unroll
                    for (uint32_t i = 0; i < kAhead; i++) q[i] = pixel_at(plf_column(i, lane));
                }
                for (uint32_t i = 0; i < PLF_K; i += kAhead) {
#pragma unroll
                    for (uint32_t u = 0; u < kAhead; u++, t++) {
                        const int64_t x = plf_column(t, lane);
                        PlfErr f;
                        f.lo = __shfl_up(s.last.lo, 1);
                        f.hi = __shfl_up(s.last.hi, 1);
                        if (lane == 0) f = above(t + 1);
                        plf_lane_shift(s, f);
                        const uint32_t p = q[u];
                        q[u] = pixel_at(x + kAhead);
                        if (has_row && x >= 0 && (uint64_t)x < W) {
                            dst[x] = plf_pixel<Visible>(pal2, entries, p, s.last, s.ul, s.up, s.ur, &s.last, nullptr, straight);
                            if (lane == PLF_LANES - 1) {
                                if (to_ring) ring[plf_ring_index(wave + 1, (uint64_t)x)] = s.last;
                                else if (to_line) j.line[x] = s.last;
                            }
                        } else {
                            s.last = zero;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kThreads) void pl_dither(const PlDitherJob *__restrict__ jobs) { dither_body<false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_dither_visible(const PlDitherJob *__restrict__ jobs) { dither_body<true>(jobs); }

} // namespace

hipError_t pl_launch_dither(const PlDitherJob *d_jobs, size_t n, hipStream_t stream, bool visible)
{
    constexpr size_t kMaxImages = (size_t)1 << 30;
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(visible ? pl_dither_visible : pl_dither, dim3((unsigned)m), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

/*
 * pl_distort.hip -- how lossy a run was, measured on the device (gfx950).  Two HBM-bound kernels around the pipeline of pl_host.hip:enqueue, both
 * one launch for the whole batch (blockIdx.y = image), like the kernels of pl_prepost.hip:
 *
 *   pl_keep     copies the original RGBA8 of every image into the context's keep arena, before pl_classify / pl_repack rewrite it in place
 *   pl_distort  behind pl_unpack: reads the kept original and the final pixels and adds the image's record up (pl_distort_core.h)
 *   pl_distort_visible  the same over visible pixels (option "measure" at "visible"): premultiplies after the load and counts the visible pixels
 *
 * pngloss_hip_compare_batch runs pl_distort alone, on two images of the caller's.  No reference equivalent.
 */
#include "pl_distort.h"

namespace {

constexpr int kThreads = PLD_THREADS, kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void pl_keep(const PlDistortJob *__restrict__ jobs)
{
    const PlDistortJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    /* 16 B per lane per load and store where both sides allow it (the arena's side always does) */
    const size_t n4 = pld_vector_quads(j.keep, j.img, n);
    const uint4 *__restrict__ src4 = reinterpret_cast<const uint4 *>(j.img);
    uint4 *__restrict__ dst4 = reinterpret_cast<uint4 *>(j.keep);
    const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, nthreads = (size_t)gridDim.x * kThreads;
    for (size_t i = tid; i < n4; i += nthreads) dst4[i] = src4[i];
    for (size_t i = n4 * 4 + tid; i < n; i += nthreads) j.keep[i] = j.img[i];
}

/* Visible: the visible mode of pl_distort_core.h -- the sums over premultiplied pixels, and the image's `pixels` is the count of visible ones, merged
 * like the other sums (the record is zeroed before the launch).  Without it: `pixels` is the job's, written once. */
template <bool Visible>
__device__ __forceinline__ void distort_body(const PlDistortJob *__restrict__ jobs)
{
    const PlDistortJob j = jobs[blockIdx.y];
    PldSum s = pld_thread<Visible>(j.keep, j.img, (size_t)j.pixels, (size_t)blockIdx.x * kThreads + threadIdx.x, (size_t)gridDim.x * kThreads);
    /* per wave, then per workgroup; then ONE atomic per quantity and workgroup, and none for a quantity that is zero (pl_classify's finding: same-address
     * atomics, one per wave, were most of that kernel's time) */
#pragma unroll
    for (int off = 32; off; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            s.sq[c] += __shfl_down(s.sq[c], off);
            s.mx[c] = max(s.mx[c], __shfl_down(s.mx[c], off));
        }
        s.changed += __shfl_down(s.changed, off);
        if (Visible) s.visible += __shfl_down(s.visible, off);
    }
    constexpr uint32_t kSums = Visible ? 6 : 5;
    __shared__ uint64_t wsum[kWaves][kSums];   /* sq[0..3], changed; visible */
    __shared__ uint32_t wmax[kWaves][4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int c = 0; c < 4; c++) { wsum[wave][c] = s.sq[c]; wmax[wave][c] = s.mx[c]; }
        wsum[wave][4] = s.changed;
        if (Visible) wsum[wave][kSums - 1] = s.visible;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 5) {
        uint64_t v = 0;
        for (int w = 0; w < kWaves; w++) v += wsum[w][t];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(t < 4 ? &j.record->sq_err[t] : &j.record->changed_pixels), (unsigned long long)v);
    } else if (t < 9) {
        uint32_t v = 0;
        for (int w = 0; w < kWaves; w++) v = max(v, wmax[w][t - 5]);
        if (v) atomicMax(&j.record->max_abs[t - 5], v);
    } else if (Visible) {
        if (t == 9) {
            uint64_t v = 0;
            for (int w = 0; w < kWaves; w++) v += wsum[w][kSums - 1];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&j.record->pixels), (unsigned long long)v);
        }
    } else if (t == 9 && blockIdx.x == 0) j.record->pixels = j.pixels;
}

__global__ __launch_bounds__(kThreads) void pl_distort(const PlDistortJob *__restrict__ jobs) { distort_body<false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_distort_visible(const PlDistortJob *__restrict__ jobs) { distort_body<true>(jobs); }

/* as pl_prepost.hip:batch_grid: enough workgroups to fill 256 CUs several times over, but never more than the batch needs; a launch takes at most
 * PLD_MAX_IMAGES images (gridDim.y).  pl_distort_core.h:pld_grid_blocks has the rule. */
constexpr size_t kMaxImages = PLD_MAX_IMAGES;
dim3 distort_grid(size_t n, uint64_t max_pixels)
{
    return dim3((unsigned)pld_grid_blocks(n, max_pixels), (unsigned)n, 1);
}

} // namespace

hipError_t pl_launch_keep(const PlDistortJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(pl_keep, distort_grid(m, max_pixels), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

hipError_t pl_launch_distort(const PlDistortJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(visible ? pl_distort_visible : pl_distort, distort_grid(m, max_pixels), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

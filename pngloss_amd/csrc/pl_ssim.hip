/*
 * pl_ssim.hip -- structural similarity of the final pixels to the kept original, measured on the device (gfx950).  One launch for the whole batch
 * (blockIdx.y = image), like pl_distort, behind it in pl_host.hip:enqueue; pngloss_hip_compare_batch_ssim runs it alone, on two images of the
 * caller's.  pl_ssim_core.h has the arithmetic and says how an image is cut into tiles, cells and windows.  No reference equivalent.
 *
 * A workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its image.  Per tile: the cells of the tile and its halo -- 16-byte loads
 * where the rows allow it, a thread per 4x4 cell -- go into the LDS table as four words per cell and channel; then every (window, channel) pair of
 * the tile is formed from its 2x2 cells (four 16-byte LDS reads) and its q is added to the thread's partial record.  A thread only ever sees
 * channel threadIdx.x % 4, so the partial record is one sum and one minimum.  At the end: through the wave (lanes of equal channel), through LDS,
 * then ONE atomic per quantity and workgroup, as in pl_distort.  pl_ssim_visible is the same over visible pixels (option "measure" at "visible").
 */
#include "pl_ssim.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
static_assert(kThreads % 4 == 0, "a thread's (window, channel) pairs must all be of one channel");

/* Visible: the visible mode of pl_ssim_core.h -- premultiplied pixels, windows without a visible pixel skipped, and the image's `windows` counted here
 * (the record starts with 0 windows): the lanes of channel 3 hold the counts, merged like the sums. */
template <bool Visible>
__device__ __forceinline__ void ssim_body(const PlSsimJob *__restrict__ jobs)
{
    __shared__ PlsCell table[PLS_TILE_CELLS * 4];
    const PlSsimJob j = jobs[blockIdx.y];
    const PlsGeom g = pls_geom(j.width, j.height);
    PlsPart p = pls_part();
    for (uint64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {      /* (the same trips for every thread of the workgroup) */
        pls_thread_cells<Visible>(table, j.a, j.b, j.width, j.height, g, tile, threadIdx.x, kThreads);
        __syncthreads();
        pls_thread_windows<Visible>(p, table, g, tile, threadIdx.x, kThreads);
        __syncthreads();
    }
    /* lanes l, l + 4, l + 8, ... hold the same channel */
#pragma unroll
    for (int off = 32; off >= 4; off >>= 1) {
        p.sum += __shfl_down(p.sum, off);
        p.mn = min(p.mn, __shfl_down(p.mn, off));
        if (Visible) p.windows += __shfl_down(p.windows, off);
    }
    __shared__ int64_t wsum[kWaves][4];
    __shared__ int32_t wmin[kWaves][4];
    __shared__ uint32_t wcnt[Visible ? kWaves : 1];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < 4) { wsum[wave][lane] = p.sum; wmin[wave][lane] = p.mn; }
    if (Visible && lane == 3) wcnt[wave] = p.windows;
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 4) {
        int64_t v = 0;
        for (int w = 0; w < kWaves; w++) v += wsum[w][t];
        /* (two's complement: adding a negative sum as an unsigned 64-bit word is the signed addition) */
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&j.record->sum_q16[t]), (unsigned long long)v);
    } else if (t < 8) {
        int32_t v = PLS_ONE;
        for (int w = 0; w < kWaves; w++) v = min(v, wmin[w][t - 4]);
        if (v < PLS_ONE) atomicMin(&j.record->min_q16[t - 4], v);
    } else if (Visible && t == 8) {
        uint64_t v = 0;
        for (int w = 0; w < kWaves; w++) v += wcnt[w];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&j.record->windows), (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kThreads) void pl_ssim(const PlSsimJob *__restrict__ jobs) { ssim_body<false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_ssim_visible(const PlSsimJob *__restrict__ jobs) { ssim_body<true>(jobs); }

/* enough workgroups to fill 256 CUs several times over, but never more than the batch needs (pl_distort.hip:distort_grid); a launch takes at most
 * PLS_MAX_IMAGES images (gridDim.y).  pl_ssim_core.h:pls_grid_blocks has the rule. */
constexpr size_t kMaxImages = PLS_MAX_IMAGES;
dim3 ssim_grid(size_t n, uint64_t max_tiles)
{
    return dim3((unsigned)pls_grid_blocks(n, max_tiles), (unsigned)n, 1);
}

} // namespace

hipError_t pl_launch_ssim(const PlSsimJob *d_jobs, size_t n, uint64_t max_tiles, hipStream_t stream, bool visible)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(visible ? pl_ssim_visible : pl_ssim, ssim_grid(m, max_tiles), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

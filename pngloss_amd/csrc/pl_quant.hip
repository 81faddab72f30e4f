/*
 * pl_quant.hip -- the colour quantiser on the device (gfx950; include/pngloss_hip_quant.h).  Kernels behind pl_host_quant.hip, each one launch for
 * its batch (blockIdx.y or .x = image); the logic is pl_quant_core.h's.
 *
 *   pl_quant_hist    every image with pixels: the 65 536-bin histogram the host's median cut reads.  16-byte loads, four pixels per lane, a run of
 *                    pixels of one bin costs one atomic
 *   pl_quant_assign  the hot kernel, once per refinement round: the palette and each entry's base in LDS (2 KiB, every lane reads the same entry: a
 *                    broadcast), per pixel and entry one v_dot4_u32_u8, one v_lshl_add_u32 and one v_max_u32; counts and channel sums in 32-bit LDS
 *                    cells of the workgroup (5 KiB), flushed with one 64-bit agent-scope atomic per non-zero cell
 *   pl_quant_remap   the same search without the accumulation: every pixel's nearest entry written to the job's `out`
 *   pl_quant_measure the remap pass in a measure-only mode (pl_quant_measure_core.h): the same search, (pixel, entry word) into the sums of a distortion
 *                    record, no pixel stored -- a probe of pngloss_hip_quantize_batch_target reads 4 bytes per pixel and writes a record
 *   pl_quant_update  one workgroup per image: the new entries from the accumulators, which it zeroes for the next round
 *
 * The rounds are enqueued back to back on one stream; no kernel waits for another workgroup.  No reference equivalent.
 */
#include "pl_quant.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kChunk = (size_t)kThreads * PLQ_QUAD;
constexpr uint32_t kCells = PLQ_MAX_COLORS * PLQ_CELLS;
static_assert(kThreads == (int)PLQ_MAX_COLORS, "one lane loads one palette entry and updates one entry");
static_assert(kCells % kThreads == 0, "the cells are walked in whole steps of the workgroup");

/* up to PLQ_QUAD words from p (16-byte load when it is aligned and whole) */
__device__ __forceinline__ void load_quad(const uint32_t *p, uint32_t m, uint32_t w[PLQ_QUAD])
{
    if (m == PLQ_QUAD && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < PLQ_QUAD; k++) w[k] = k < m ? p[k] : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void pl_quant_hist(const PlQuantJob *__restrict__ jobs)
{
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    for (size_t c = blockIdx.x; c * kChunk < n; c += gridDim.x) {
        const size_t base = c * kChunk + (size_t)threadIdx.x * PLQ_QUAD;
        if (base >= n) continue;
        const uint32_t m = n - base < PLQ_QUAD ? (uint32_t)(n - base) : PLQ_QUAD;
        uint32_t w[PLQ_QUAD];
        load_quad(j.img + base, m, w);
        plq_hist_quad(j.hist, w, m);
    }
}

/* Remap: no accumulation, the nearest entry's word stored per pixel */
template <bool Remap>
__device__ __forceinline__ void assign_body(const PlQuantJob *__restrict__ jobs)
{
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    __shared__ uint32_t cells[Remap ? 1 : kCells];
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    if ((size_t)blockIdx.x * kChunk >= n) return;       /* the whole workgroup: the grid is sized by the largest image of the launch */
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    if (threadIdx.x < entries) {
        const uint32_t word = j.pal[threadIdx.x];
        pal2[2 * threadIdx.x] = word;
        pal2[2 * threadIdx.x + 1] = plq_base(word, threadIdx.x);
    }
    if (!Remap)
        for (uint32_t i = threadIdx.x; i < kCells; i += kThreads) cells[i] = 0;
    __syncthreads();
    for (size_t c = blockIdx.x; c * kChunk < n; c += gridDim.x) {
        const size_t base = c * kChunk + (size_t)threadIdx.x * PLQ_QUAD;
        if (base >= n) continue;
        const uint32_t m = n - base < PLQ_QUAD ? (uint32_t)(n - base) : PLQ_QUAD;
        uint32_t w[PLQ_QUAD], best[PLQ_QUAD];
        load_quad(j.img + base, m, w);
        plq_search_quad(pal2, entries, w, m, best);
        if (Remap) {
            uint32_t *dst = j.out + base;
            if (m == PLQ_QUAD && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0)
                *reinterpret_cast<uint4 *>(dst) = make_uint4(pal2[2 * best[0]], pal2[2 * best[1]], pal2[2 * best[2]], pal2[2 * best[3]]);
            else
                for (uint32_t k = 0; k < m; k++) dst[k] = pal2[2 * best[k]];
        } else {
            plq_accumulate_quad(cells, w, best, m);
        }
    }
    if (!Remap) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < kCells; i += kThreads) plq_flush_cell(j.acc, cells, i);
    }
}

__global__ __launch_bounds__(kThreads) void pl_quant_assign(const PlQuantJob *__restrict__ jobs) { assign_body<false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_quant_remap(const PlQuantJob *__restrict__ jobs) { assign_body<true>(jobs); }

/* The record of job k is records[k], zeroed before the launch; `pixels` is the host's to write.  A workgroup takes up to PLQ_WG_PIXELS pixels
 * (plq_blocks), a lane of it so up to PLQ_WG_PIXELS / kThreads -- more than a lane's 32-bit sums hold, which is why plq_measure_lane flushes them. */
static_assert(PLQ_WG_PIXELS / kThreads + PLQ_QUAD > PLD_FLUSH_PIXELS, "a lane of pl_quant_measure can pass PLD_FLUSH_PIXELS pixels: its sums are flushed, not merely bounded");
__global__ __launch_bounds__(kThreads) void pl_quant_measure(const PlQuantJob *__restrict__ jobs, PlDistortRecord *__restrict__ records)
{
    constexpr int kWaves = kThreads / 64;
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    __shared__ uint64_t wsum[kWaves][5];        /* sq[0..3], changed */
    __shared__ uint32_t wmax[kWaves][4];
    const PlQuantJob j = jobs[blockIdx.y];
    PlDistortRecord *const record = records + blockIdx.y;
    const size_t n = (size_t)j.pixels;
    if ((size_t)blockIdx.x * kChunk >= n) return;       /* the whole workgroup: the grid is sized by the largest image of the launch */
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    if (threadIdx.x < entries) {
        const uint32_t word = j.pal[threadIdx.x];
        pal2[2 * threadIdx.x] = word;
        pal2[2 * threadIdx.x + 1] = plq_base(word, threadIdx.x);
    }
    __syncthreads();
    PldSum s = plq_measure_lane(pal2, entries, j.img, n, blockIdx.x, gridDim.x, threadIdx.x, kThreads);
    /* per wave, then per workgroup; then ONE atomic per quantity and workgroup, none for a quantity that is zero: as pl_distort merges them */
#pragma unroll
    for (int off = 32; off; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            s.sq[c] += __shfl_down(s.sq[c], off);
            s.mx[c] = max(s.mx[c], __shfl_down(s.mx[c], off));
        }
        s.changed += __shfl_down(s.changed, off);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int c = 0; c < 4; c++) { wsum[wave][c] = s.sq[c]; wmax[wave][c] = s.mx[c]; }
        wsum[wave][4] = s.changed;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 5) {
        uint64_t v = 0;
        for (int w = 0; w < kWaves; w++) v += wsum[w][t];
        if (v) PLQ_ADD64(t < 4 ? &record->sq_err[t] : &record->changed_pixels, v);
    } else if (t < 9) {
        uint32_t v = 0;
        for (int w = 0; w < kWaves; w++) v = max(v, wmax[w][t - 5]);
        if (v) atomicMax(&record->max_abs[t - 5], v);
    }
}

__global__ __launch_bounds__(kThreads) void pl_quant_update(const PlQuantJob *__restrict__ jobs)
{
    const PlQuantJob j = jobs[blockIdx.x];
    plq_update_entry(j.pal, j.acc, threadIdx.x);        /* (an entry past `entries` has no count: its accumulator is zeroed, its word stays) */
}

constexpr size_t kMaxImages = 65535;                /* gridDim.y */

/* enough workgroups to fill 256 CUs a few times over, never more than the largest image has chunks, never so few that a workgroup's 32-bit cells
 * could overflow (plq_blocks) */
dim3 quant_grid(size_t m, uint64_t max_pixels)
{
    size_t want = (2048 + m - 1) / m;
    if (want < 8) want = 8;
    return dim3(plq_blocks(max_pixels, kChunk, (uint32_t)want), (unsigned)m, 1);
}

template <class Kernel>
hipError_t launch_over_pixels(Kernel kernel, const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream)
{
    if (!plq_pixels_ok(max_pixels)) return hipErrorInvalidValue;
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(kernel, quant_grid(m, max_pixels), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

} // namespace

hipError_t pl_launch_quant_hist(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream) { return launch_over_pixels(pl_quant_hist, d_jobs, n, max_pixels, stream); }
hipError_t pl_launch_quant_assign(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream) { return launch_over_pixels(pl_quant_assign, d_jobs, n, max_pixels, stream); }
hipError_t pl_launch_quant_remap(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream) { return launch_over_pixels(pl_quant_remap, d_jobs, n, max_pixels, stream); }

hipError_t pl_launch_quant_measure(const PlQuantJob *d_jobs, PlDistortRecord *d_records, size_t n, uint64_t max_pixels, hipStream_t stream)
{
    if (!plq_pixels_ok(max_pixels)) return hipErrorInvalidValue;
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(pl_quant_measure, quant_grid(m, max_pixels), dim3(kThreads), 0, stream, d_jobs + first, d_records + first);
    }
    return hipGetLastError();
}

hipError_t pl_launch_quant_update(const PlQuantJob *d_jobs, size_t n, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(pl_quant_update, dim3((unsigned)m), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

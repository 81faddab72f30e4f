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
 *   pl_quant_hist_visible, pl_quant_assign_visible, pl_quant_remap_visible, pl_quant_measure_visible
 *                    the same kernels in the premultiplied space (include/pngloss_hip_quant_space.h): a pixel is premultiplied once behind its load,
 *                    the palette holds premultiplied words, and the remap stores the straight word of the nearest entry from a second LDS table
 *                    (1 KiB; lane e makes entry e's word at the kernel's start: three divisions per entry, none per pixel).  pl_quant_update serves
 *                    both spaces
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

/* Visible: bin 0 of the premultiplied histogram takes every pixel that is all but invisible; a lane counts its own (plq_hist_quad: held0), the wave
 * adds them up and leaves one atomic (measured on a frame with a third of its pixels at alpha 0: 49.5 ms with an atomic per quad) */
template <bool Visible>
__device__ __forceinline__ void hist_body(const PlQuantJob *__restrict__ jobs)
{
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    uint32_t held0 = 0;
    for (size_t c = blockIdx.x; c * kChunk < n; c += gridDim.x) {
        const size_t base = c * kChunk + (size_t)threadIdx.x * PLQ_QUAD;
        if (base >= n) continue;
        const uint32_t m = n - base < PLQ_QUAD ? (uint32_t)(n - base) : PLQ_QUAD;
        uint32_t w[PLQ_QUAD];
        load_quad(j.img + base, m, w);
        plq_hist_quad<Visible>(j.hist, w, m, Visible ? &held0 : nullptr);
    }
    if (Visible) {
#pragma unroll
        for (int off = 32; off; off >>= 1) held0 += __shfl_down(held0, off);
        if ((threadIdx.x & 63) == 0 && held0) PLQ_ADD32(j.hist, held0);
    }
}

__global__ __launch_bounds__(kThreads) void pl_quant_hist(const PlQuantJob *__restrict__ jobs) { hist_body<false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_quant_hist_visible(const PlQuantJob *__restrict__ jobs) { hist_body<true>(jobs); }

/* the remap pass of the premultiplied space keeps the straight word of every entry; the other kernels have no such table */
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

/* Remap: no accumulation, the nearest entry's word stored per pixel.  Visible: the search on premultiplied pixels, the word stored the straight one */
template <bool Remap, bool Visible>
__device__ __forceinline__ void assign_body(const PlQuantJob *__restrict__ jobs)
{
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    __shared__ uint32_t cells[Remap ? 1 : kCells];
    uint32_t *const straight = straight_table<Remap && Visible>();
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    if ((size_t)blockIdx.x * kChunk >= n) return;       /* the whole workgroup: the grid is sized by the largest image of the launch */
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    if (threadIdx.x < entries) {
        const uint32_t word = j.pal[threadIdx.x];
        pal2[2 * threadIdx.x] = word;
        pal2[2 * threadIdx.x + 1] = plq_base(word, threadIdx.x);
        if (Remap && Visible) straight[threadIdx.x] = plq_straight(word);
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
        plq_space_quad<Visible>(w, m);
        plq_search_quad(pal2, entries, w, m, best);
        if (Remap && Visible) {
            uint32_t *dst = j.out + base;
            if (m == PLQ_QUAD && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0)
                *reinterpret_cast<uint4 *>(dst) = make_uint4(straight[best[0]], straight[best[1]], straight[best[2]], straight[best[3]]);
            else
                for (uint32_t k = 0; k < m; k++) dst[k] = straight[best[k]];
        } else if (Remap) {
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

__global__ __launch_bounds__(kThreads) void pl_quant_assign(const PlQuantJob *__restrict__ jobs) { assign_body<false, false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_quant_remap(const PlQuantJob *__restrict__ jobs) { assign_body<true, false>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_quant_assign_visible(const PlQuantJob *__restrict__ jobs) { assign_body<false, true>(jobs); }
__global__ __launch_bounds__(kThreads) void pl_quant_remap_visible(const PlQuantJob *__restrict__ jobs) { assign_body<true, true>(jobs); }

/* a lane's sums into the image's record: per wave, then per workgroup; then ONE atomic per quantity and workgroup, none for a quantity that is
 * zero: as pl_distort merges them.  Visible: the count of visible pixels into `pixels` too */
template <bool Visible>
__device__ __forceinline__ void measure_merge(PldSum s, PlDistortRecord *record)
{
    constexpr int kWaves = kThreads / 64;
    constexpr uint32_t kSums = Visible ? 6 : 5;
    __shared__ uint64_t wsum[kWaves][kSums];    /* sq[0..3], changed; visible */
    __shared__ uint32_t wmax[kWaves][4];
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
        if (v) PLQ_ADD64(t < 4 ? &record->sq_err[t] : &record->changed_pixels, v);
    } else if (t < 9) {
        uint32_t v = 0;
        for (int w = 0; w < kWaves; w++) v = max(v, wmax[w][t - 5]);
        if (v) atomicMax(&record->max_abs[t - 5], v);
    } else if (Visible && t == 9) {
        uint64_t v = 0;
        for (int w = 0; w < kWaves; w++) v += wsum[w][kSums - 1];
        if (v) PLQ_ADD64(&record->pixels, v);
    }
}

/* The record of job k is records[k], zeroed before the launch; `pixels` is the host's to write.  A workgroup takes up to PLQ_WG_PIXELS pixels
 * (plq_blocks), a lane of it so up to PLQ_WG_PIXELS / kThreads -- more than a lane's 32-bit sums hold, which is why plq_measure_lane flushes them. */
static_assert(PLQ_WG_PIXELS / kThreads + PLQ_QUAD > PLD_FLUSH_PIXELS, "a lane of pl_quant_measure can pass PLD_FLUSH_PIXELS pixels: its sums are flushed, not merely bounded");
__global__ __launch_bounds__(kThreads) void pl_quant_measure(const PlQuantJob *__restrict__ jobs, PlDistortRecord *__restrict__ records)
{
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    if ((size_t)blockIdx.x * kChunk >= n) return;       /* the whole workgroup: the grid is sized by the largest image of the launch */
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    if (threadIdx.x < entries) {
        const uint32_t word = j.pal[threadIdx.x];
        pal2[2 * threadIdx.x] = word;
        pal2[2 * threadIdx.x + 1] = plq_base(word, threadIdx.x);
    }
    __syncthreads();
    measure_merge<false>(plq_measure_lane(pal2, entries, j.img, n, blockIdx.x, gridDim.x, threadIdx.x, kThreads), records + blockIdx.y);
}

/* the same in the premultiplied space: the visible-mode record of (input, remapped image), `pixels` -- the visible ones -- counted here */
__global__ __launch_bounds__(kThreads) void pl_quant_measure_visible(const PlQuantJob *__restrict__ jobs, PlDistortRecord *__restrict__ records)
{
    __shared__ uint32_t pal2[2 * PLQ_MAX_COLORS];
    const PlQuantJob j = jobs[blockIdx.y];
    const size_t n = (size_t)j.pixels;
    if ((size_t)blockIdx.x * kChunk >= n) return;
    const uint32_t entries = j.entries < PLQ_MAX_COLORS ? j.entries : PLQ_MAX_COLORS;
    if (threadIdx.x < entries) {
        const uint32_t word = j.pal[threadIdx.x];
        pal2[2 * threadIdx.x] = word;
        pal2[2 * threadIdx.x + 1] = plq_base(word, threadIdx.x);
    }
    __syncthreads();
    measure_merge<true>(plq_measure_lane<true>(pal2, entries, j.img, n, blockIdx.x, gridDim.x, threadIdx.x, kThreads), records + blockIdx.y);
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

hipError_t pl_launch_quant_hist(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible)
{
    return launch_over_pixels(visible ? pl_quant_hist_visible : pl_quant_hist, d_jobs, n, max_pixels, stream);
}
hipError_t pl_launch_quant_assign(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible)
{
    return launch_over_pixels(visible ? pl_quant_assign_visible : pl_quant_assign, d_jobs, n, max_pixels, stream);
}
hipError_t pl_launch_quant_remap(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible)
{
    return launch_over_pixels(visible ? pl_quant_remap_visible : pl_quant_remap, d_jobs, n, max_pixels, stream);
}

hipError_t pl_launch_quant_measure(const PlQuantJob *d_jobs, PlDistortRecord *d_records, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible)
{
    if (!plq_pixels_ok(max_pixels)) return hipErrorInvalidValue;
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        hipLaunchKernelGGL(visible ? pl_quant_measure_visible : pl_quant_measure, quant_grid(m, max_pixels), dim3(kThreads), 0, stream, d_jobs + first, d_records + first);
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

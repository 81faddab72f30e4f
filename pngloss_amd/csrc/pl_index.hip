/*
 * pl_index.hip -- the indexed-colour write side on the device (gfx950; option "indexed", include/pngloss_hip.h).  Three kernels behind the
 * pipeline of pl_host_window.hip:window_index, each one launch for its batch (blockIdx.y or .x = image); the logic is pl_index_core.h's.
 *
 *   pl_index_count    every image: its distinct RGBA words into a per-image open-addressing table, with an early exit.  A workgroup takes chunks
 *                     of kChunk pixels; before each it re-reads the image's counter and leaves once that is past 256, and so does every lane
 *                     before it touches the table -- a photograph is done after its first few thousand pixels.  A word equal to the pixel before
 *                     it is skipped, the others go through a 256-entry LDS pre-filter, so that a flat image does not hammer one global slot.
 *   pl_index_palette  one workgroup per eligible image: gathers the table's <= 256 words, rank-sorts them, writes the palette record and each
 *                     colour's index beside it in its slot
 *   pl_index_rows     eligible images: the table in LDS (8 KB), four lookups per lane packed into one dword store; one zero filter byte per row
 *   pl_index_pack     option "index_depth" at "auto" or "min" only, eligible images of at most 16 colours: the 8-bit index rows packed at bit depth
 *                     1, 2 or 4 (the job says which: one launch for a batch that mixes them), a lane one dword of a packed row from 16-byte
 *                     loads; no table, no LDS; one zero filter byte per row
 *
 * No kernel waits on another workgroup: the only cross-workgroup traffic is the compare-and-swap on a slot and the relaxed counter.
 * No reference equivalent.
 */
#include "pl_index.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kChunk = (size_t)kThreads * PLI_QUAD;
static_assert(kThreads == (int)PLI_CACHE, "pl_index_count: one lane clears one entry of the pre-filter");
static_assert(PLI_SLOTS % kThreads == 0, "the table is walked in whole steps of the workgroup");

/* up to PLI_QUAD words from p (16-byte load when it is aligned and whole) */
__device__ __forceinline__ void load_quad(const uint32_t *p, uint32_t m, uint32_t w[PLI_QUAD])
{
    if (m == PLI_QUAD && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < PLI_QUAD; k++) w[k] = k < m ? p[k] : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void pl_index_count(const PlIndexJob *__restrict__ jobs)
{
    __shared__ uint64_t cache[PLI_CACHE];
    __shared__ uint32_t seen[2];
    const PlIndexJob j = jobs[blockIdx.y];
    cache[threadIdx.x] = PLI_EMPTY;
    const size_t n = (size_t)j.pixels;
    uint32_t turn = 0;
    for (size_t c = blockIdx.x; c * kChunk < n; c += gridDim.x, turn ^= 1u) {
        if (threadIdx.x == 0) seen[turn] = PLI_LOAD32(j.count);
        __syncthreads();                            /* (the first one also ends the clearing of the pre-filter) */
        if (seen[turn] > PLI_MAX_COLORS) return;    /* the whole workgroup: the image is not eligible, nothing else is asked of this kernel */
        const size_t base = c * kChunk + (size_t)threadIdx.x * PLI_QUAD;
        if (base < n) {
            const uint32_t m = n - base < PLI_QUAD ? (uint32_t)(n - base) : PLI_QUAD;
            uint32_t w[PLI_QUAD];
            load_quad(j.img + base, m, w);
            pli_count_quad(j.table, j.count, cache, w, m, base != 0, base ? j.img[base - 1] : 0u);
        }
    }
}

__global__ __launch_bounds__(kThreads) void pl_index_palette(const PlIndexJob *__restrict__ jobs)
{
    __shared__ uint32_t list_word[PLI_MAX_COLORS], list_slot[PLI_MAX_COLORS], m;
    const PlIndexJob j = jobs[blockIdx.x];
    if (threadIdx.x == 0) m = 0;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < PLI_SLOTS; s += kThreads) pli_collect(j.table, s, list_word, list_slot, &m);
    __syncthreads();
    const uint32_t entries = m < PLI_MAX_COLORS ? m : PLI_MAX_COLORS;
    if (threadIdx.x < entries) pli_assign(j.table, list_word, list_slot, entries, threadIdx.x, j.record);
    if (threadIdx.x == 0) j.record->entries = m;    /* (the host holds it against the counter) */
}

__global__ __launch_bounds__(kThreads) void pl_index_rows(const PlIndexJob *__restrict__ jobs)
{
    __shared__ uint64_t table[PLI_SLOTS];
    const PlIndexJob j = jobs[blockIdx.y];
    if (blockIdx.x >= j.height) return;
    for (uint32_t s = threadIdx.x; s < PLI_SLOTS; s += kThreads) table[s] = j.table[s];
    __syncthreads();
    const uint32_t W = j.width, quads = (W + PLI_QUAD - 1) / PLI_QUAD;      /* quads * 4 <= pitch: the tail's dword stays inside the row */
    for (uint32_t y = blockIdx.x; y < j.height; y += gridDim.x) {
        if (threadIdx.x == 0) j.ids[y] = 0;
        const uint32_t *row = j.img + (size_t)y * W;
        uint32_t *dst = reinterpret_cast<uint32_t *>(j.rows + (size_t)y * j.pitch);
        for (uint32_t q = threadIdx.x; q < quads; q += kThreads) {
            const uint32_t x = q * PLI_QUAD, m = W - x < PLI_QUAD ? W - x : PLI_QUAD;
            uint32_t w[PLI_QUAD];
            load_quad(row + x, m, w);
            dst[q] = pli_pack_quad(table, w, m);
        }
    }
}

/* the rows of one job packed at depth D: a workgroup strides over the rows, a lane over the dwords of a packed row (256 lanes make 8192 / 4096 /
 * 2048 pixels a trip at depth 1 / 2 / 4) */
template <uint32_t D> __device__ __forceinline__ void pack_rows(const PlPackJob &j)
{
    const uint32_t dwords = pli_packed_dwords(j.width, D);                   /* dwords * 4 <= pitch: the tail's dword stays inside the row */
    for (uint32_t y = blockIdx.x; y < j.height; y += gridDim.x) {
        if (threadIdx.x == 0) j.ids[y] = 0;
        const uint8_t *row8 = j.rows8 + (size_t)y * j.pitch8;
        uint32_t *dst = reinterpret_cast<uint32_t *>(j.rows + (size_t)y * j.pitch);
        for (uint32_t q = threadIdx.x; q < dwords; q += kThreads) dst[q] = pli_pack_lane<D>(row8, j.width, q);
    }
}

__global__ __launch_bounds__(kThreads) void pl_index_pack(const PlPackJob *__restrict__ jobs)
{
    const PlPackJob j = jobs[blockIdx.y];
    if (j.depth == 1) pack_rows<1>(j);                /* (uniform for the workgroup: the job is blockIdx.y's) */
    else if (j.depth == 2) pack_rows<2>(j);
    else if (j.depth == 4) pack_rows<4>(j);
}

constexpr size_t kMaxImages = 65535;                /* gridDim.y */

} // namespace

hipError_t pl_launch_index_count(const PlIndexJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        /* few workgroups per image: the lanes that are inside their first insertion when the counter passes 256 are what a non-eligible image
         * costs (measured on one 1920x1080 photograph: 279 us with up to 128 workgroups and a counter check every 32 probes) */
        size_t blocks = (size_t)((max_pixels + kChunk - 1) / kChunk), cap = (32 + m - 1) / m;
        if (cap < 8) cap = 8;
        if (blocks > cap) blocks = cap;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(pl_index_count, dim3((unsigned)blocks, (unsigned)m), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

hipError_t pl_launch_index_palette(const PlIndexJob *d_jobs, size_t n, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(pl_index_palette, dim3((unsigned)n), dim3(kThreads), 0, stream, d_jobs);
    return hipGetLastError();
}

hipError_t pl_launch_index_rows(const PlIndexJob *d_jobs, size_t n, uint32_t max_height, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        uint32_t blocks = max_height < 512 ? max_height : 512;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(pl_index_rows, dim3(blocks, (unsigned)m), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

hipError_t pl_launch_index_pack(const PlPackJob *d_jobs, size_t n, uint32_t max_height, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxImages) {
        const size_t m = n - first < kMaxImages ? n - first : kMaxImages;
        uint32_t blocks = max_height < 512 ? max_height : 512;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(pl_index_pack, dim3(blocks, (unsigned)m), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

/*
 * pl_prepost.hip -- the fully data-parallel, HBM-bound kernels around the row engine (gfx950).
 *
 *   pl_init      zero/seed the per-image workspace
 *   pl_classify  gray / opaque detection            (replaces pngloss_image.c:64-80, without the early exit)
 *   pl_repack    RGBA8 -> "slots" layout in place   (replaces pngloss_image.c:81-124)
 *   pl_hist      original_frequency[5][256]         (replaces optimize_state.c:66-83, computed once, not 3x)
 *   pl_rank      8-bit order-preserving rank of each original_frequency table (new: lets the row engine compare
 *                the secondary key of optimize_state.c:228-231 inside one 32-bit arg-max word)
 *   pl_unpack    "slots" -> RGBA8 in place           (replaces pngloss_image.c:125-148)
 *
 * One launch covers the whole batch: blockIdx.y = image.  The class (bytes per pixel) is decided on the device and
 * read back from PlJob::flags by every later kernel, so the host never synchronises inside the pipeline.
 */
#include "pl_device.h"
#include "pl_prepost_core.h"
#include <cstdlib>

namespace {

constexpr int kThreads = PLP_THREADS;

__global__ __launch_bounds__(kThreads) void pl_init(const PlJob *jobs)
{
    const PlJob j = jobs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        *j.flags = PL_FLAG_GRAY | PL_FLAG_OPAQUE;
        *j.out_flags = PL_FLAG_GRAY | PL_FLAG_OPAQUE;
        for (int r = 0; r < PLR_WORDS; r++) j.result[r] = 0;
    }
    for (uint32_t i = t; i < PL_NFILT * PL_NSYM; i += kThreads) j.orig_hist[i] = 0;
    for (uint32_t i = t; i < j.width; i += kThreads) {
        j.err0[i] = make_uint2(0, 0);
        j.err1[i] = make_uint2(0, 0);
        j.old_above[i] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void pl_classify(const PlJob *jobs)
{
    const PlJob j = jobs[blockIdx.y];
    if (j.forced_bpp) return;
    const size_t n = (size_t)j.width * j.height;
    uint32_t gray = 1, opaque = 1;
    /* 16 B per lane per load when the pixel count allows it */
    const size_t n4 = (reinterpret_cast<uintptr_t>(j.img) & 15u) ? 0 : n / 4;
    const uint4 *p4 = reinterpret_cast<const uint4 *>(j.img);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)gridDim.x * kThreads) {
        const uint4 v = p4[i];
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t r = w[k] & 255u, g = (w[k] >> 8) & 255u, b = (w[k] >> 16) & 255u, a = w[k] >> 24;
            gray &= (r == g) & (g == b);
            opaque &= (a == 255u);
        }
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const uint32_t w = j.img[i];
        const uint32_t r = w & 255u, g = (w >> 8) & 255u, b = (w >> 16) & 255u, a = w >> 24;
        gray &= (r == g) & (g == b);
        opaque &= (a == 255u);
    }
    /* one atomic per WORKGROUP at most (8192 same-address atomics, one per wave, used to cost 80 us of a 100 us kernel),
     * and none at all once the flag word already says "neither gray nor opaque" */
    __shared__ uint32_t wg_clear;
    if (threadIdx.x == 0) wg_clear = 0;
    __syncthreads();
    const bool all_gray = __all(gray), all_opaque = __all(opaque);
    if ((threadIdx.x & 63) == 0) {
        const uint32_t clear = (all_gray ? 0u : PL_FLAG_GRAY) | (all_opaque ? 0u : PL_FLAG_OPAQUE);
        if (clear) atomicOr(&wg_clear, clear);
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_clear) {
        const uint32_t now = __hip_atomic_load(j.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (now & wg_clear) atomicAnd(j.flags, ~wg_clear);
    }
}

__global__ __launch_bounds__(kThreads) void pl_repack(const PlJob *jobs)
{
    const PlJob j = jobs[blockIdx.y];
    if (j.forced_bpp) return;
    const uint32_t bpp = pl_bpp_from_flags(*j.flags);
    if (bpp == 4) return;
    const size_t n = (size_t)j.width * j.height;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const uint32_t w = j.img[i];
        uint32_t o;
        if (bpp == 3) o = w & 0x00ffffffu;                       /* r,g,b,0 */
        else if (bpp == 2) o = ((w >> 8) & 255u) | ((w >> 24) << 8); /* g,a,0,0 : gray is the G channel (pngloss_image.c:112-115) */
        else o = (w >> 8) & 255u;                                 /* g,0,0,0 */
        j.img[i] = o;
    }
}

__global__ __launch_bounds__(kThreads) void pl_unpack(const PlJob *jobs)
{
    const PlJob j = jobs[blockIdx.y];
    if (j.forced_bpp) return;
    const uint32_t bpp = pl_bpp_from_flags(*j.flags);
    if (bpp == 4) return;
    const size_t n = (size_t)j.width * j.height;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const uint32_t w = j.img[i];
        uint32_t o;
        if (bpp == 3) o = w | 0xff000000u;
        else {
            const uint32_t g = w & 255u;
            const uint32_t a = bpp == 2 ? ((w >> 8) & 255u) : 255u;
            o = g | (g << 8) | (g << 16) | (a << 24);
        }
        j.img[i] = o;
    }
}

/* original_frequency: for every channel byte and each of the five predictors, count (byte - prediction) mod 256,
 * predictions taken from the ORIGINAL neighbours.  LDS-privatised per workgroup, one global atomic per non-empty
 * bin per workgroup at the end.
 *
 * What bounds it is the rate at which a CU retires LDS atomics (20 per pixel) and, next to that, the VALU work per pixel -- not
 * HBM.  So: REP lane-interleaved replicas of the 1280 counters, replicas of one bin in CONSECUTIVE words (different banks; natural
 * images put most residuals into a handful of bins, a wave's lanes would serialise on one word otherwise); a thread takes four
 * neighbouring pixels (one 16-byte load per row, left / diagonal neighbours from registers); sub, up and average residuals of the
 * four channel bytes are taken in one 32-bit word (byte-wise arithmetic without carries across bytes). */
template <int REP, int NCH>
__device__ __forceinline__ void pl_hist_count(uint32_t *mine, uint32_t here, uint32_t left, uint32_t above, uint32_t diag)
{
    const PlpResidual r = plp_residual(here, left, above);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        uint32_t bin[PL_NFILT];
        plp_bins(bin, c, here, left, above, diag, r);
#pragma unroll
        for (int f = 0; f < PL_NFILT; f++) atomicAdd(&mine[((uint32_t)f * PL_NSYM + bin[f]) * REP], 1u);
    }
}
/* (pl_prepost_core.h has the loop: the quad loader or the pixel loader, at the stride of the image's workgroups) */
template <int REP, int NT, int NCH>
__device__ __forceinline__ void pl_hist_loop(uint32_t *mine, const uint32_t *__restrict__ img, uint32_t W, size_t n)
{
    plp_hist_thread(img, W, n, blockIdx.x, threadIdx.x, gridDim.x, NT,
                    [mine](uint32_t here, uint32_t left, uint32_t above, uint32_t diag) { pl_hist_count<REP, NCH>(mine, here, left, above, diag); });
}
template <int REP, int NT>
__global__ __launch_bounds__(NT) void pl_hist(const PlJob *__restrict__ jobs)
{
    extern __shared__ __align__(16) uint32_t pl_hist_lds[];               /* [PL_NFILT * PL_NSYM][REP] */
    uint32_t *const h = pl_hist_lds;
    const PlJob j = jobs[blockIdx.y];
    const uint32_t bpp = pl_job_bpp(j);
    for (uint32_t i = threadIdx.x; i < REP * PL_NFILT * PL_NSYM; i += NT) h[i] = 0;
    __syncthreads();
    uint32_t *const mine = h + (threadIdx.x & (REP - 1));
    const size_t n = (size_t)j.width * j.height;
    if (bpp == 4) pl_hist_loop<REP, NT, 4>(mine, j.img, j.width, n);
    else if (bpp == 3) pl_hist_loop<REP, NT, 3>(mine, j.img, j.width, n);
    else if (bpp == 2) pl_hist_loop<REP, NT, 2>(mine, j.img, j.width, n);
    else pl_hist_loop<REP, NT, 1>(mine, j.img, j.width, n);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < PL_NFILT * PL_NSYM; i += NT) {
        uint32_t v = 0;
#pragma unroll
        for (int r = 0; r < REP; r++) v += h[i * REP + r];
        if (v) atomicAdd(&j.orig_hist[i], v);
    }
}

/* rank[f][b] = #{ b' : orig_hist[f][b'] < orig_hist[f][b] }  (0..255; pl_prepost_core.h:plp_rank says why that is enough) */
__global__ __launch_bounds__(PL_NSYM) void pl_rank(const PlJob *jobs)
{
    __shared__ uint32_t h[PL_NSYM];
    const PlJob j = jobs[blockIdx.x];
    for (int f = 0; f < PL_NFILT; f++) {
        const uint32_t mine = j.orig_hist[f * PL_NSYM + threadIdx.x];
        __syncthreads();
        h[threadIdx.x] = mine;
        __syncthreads();
        j.orig_rank[f * PL_NSYM + threadIdx.x] = plp_rank(h, mine);
    }
}

size_t batch_max_px(const PlJob *h_jobs, size_t n)
{
    size_t max_px = 1;
    for (size_t i = 0; i < n; i++) {
        const size_t px = (size_t)h_jobs[i].width * h_jobs[i].height;
        if (px > max_px) max_px = px;
    }
    return max_px;
}

/* one of pl_classify, pl_repack, pl_unpack over the batch: blockIdx.y = image, so a launch takes PLP_MAX_IMAGES of them and starts at its own jobs;
 * the workgroups per image are pl_prepost_core.h:plp_batch_blocks of the slice */
void launch_batch(void (*kernel)(const PlJob *), const PlJob *d_jobs, size_t n, size_t max_px, uint32_t px_per_thread, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += PLP_MAX_IMAGES) {
        const size_t m = plp_slice(n, first);
        hipLaunchKernelGGL(kernel, dim3((unsigned)plp_batch_blocks(m, max_px, px_per_thread), (unsigned)m, 1), dim3(kThreads), 0, stream, d_jobs + first);
    }
}

/* pl_hist: 16 replicas (80 KB) and 1024 threads, one workgroup per CU, three rounds of workgroups on a large frame -- measured
 * against 4 / 8 replicas, 256 / 512 threads and 256 ... 2048 workgroups in profiles/r03_hist_variants.txt */
template <int REP, int NT>
hipError_t launch_hist_v(const PlJob *d_jobs, size_t n, size_t max_px, hipStream_t stream, unsigned wgs_per_image_cap)
{
    constexpr size_t lds = (size_t)REP * PL_NFILT * PL_NSYM * sizeof(uint32_t);
    static std::atomic<unsigned> optin{ 0 };                  /* (per device: pl_lds_optin) */
    if (lds > 65536) { const hipError_t attr = pl_lds_optin(reinterpret_cast<const void *>(&pl_hist<REP, NT>), lds, optin); if (attr != hipSuccess) return attr; }
    for (size_t first = 0; first < n; first += PLP_MAX_IMAGES) {
        const size_t m = plp_slice(n, first);
        hipLaunchKernelGGL((pl_hist<REP, NT>), dim3((unsigned)plp_hist_blocks(m, max_px, NT, wgs_per_image_cap), (unsigned)m), dim3(NT), lds, stream, d_jobs + first);
    }
    return hipGetLastError();
}
hipError_t launch_hist(const PlJob *d_jobs, size_t n, size_t max_px, hipStream_t stream)
{
    static const int variant = [] { const char *e = getenv("PNGLOSS_HIP_HIST"); return e ? atoi(e) : 0; }();
    if (variant == 1) return launch_hist_v<8, 256>(d_jobs, n, max_px, stream, 2048);      /* round 2's shape, for comparison */
    return launch_hist_v<16, 1024>(d_jobs, n, max_px, stream, 768);
}

} // namespace

hipError_t pl_launch_prepare(const PlJob *d_jobs, const PlJob *h_jobs, size_t n, hipStream_t stream, bool with_hist)
{
    if (!n) return hipSuccess;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(pl_init, dim3((unsigned)n), dim3(kThreads), 0, stream, d_jobs);
    const size_t max_px = batch_max_px(h_jobs, n);
    launch_batch(pl_classify, d_jobs, n, max_px, 16, stream);
    launch_batch(pl_repack, d_jobs, n, max_px, 8, stream);
    if (!with_hist) return hipGetLastError();
    {
        e = launch_hist(d_jobs, n, max_px, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pl_rank, dim3((unsigned)n), dim3(PL_NSYM), 0, stream, d_jobs);
    return hipGetLastError();
}

hipError_t pl_launch_finish(const PlJob *d_jobs, const PlJob *h_jobs, size_t n, hipStream_t stream)
{
    if (!n) return hipSuccess;
    launch_batch(pl_unpack, d_jobs, n, batch_max_px(h_jobs, n), 8, stream);
    return hipGetLastError();
}

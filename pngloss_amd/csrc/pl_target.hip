/*
 * pl_target.hip -- the one kernel pngloss_hip_optimize_batch_target adds (gfx950): pl_move, a batched copy.  blockIdx.y selects a job {src, dst,
 * bytes} (pl_move_core.h); one launch saves the originals of a batch into the search arena, puts originals back in front of a probe, stashes the
 * accepted probes' pixels and row filters, or puts the kept results back at the end.  HBM-bound, shaped like pl_keep (pl_distort.hip).
 * The search itself is pl_target.h (host decisions) and pl_host_search.hip (the rounds); measuring is pl_distort.  No reference equivalent.
 */
#include "pl_target_dev.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void pl_move(const PlMoveJob *__restrict__ jobs)
{
    const PlMoveJob j = jobs[blockIdx.y];
    plm_thread(j.src, j.dst, (size_t)j.bytes, (size_t)blockIdx.x * kThreads + threadIdx.x, (size_t)gridDim.x * kThreads);
}

/* as pl_distort.hip:distort_grid: 256 bytes per thread and pass, enough workgroups to fill the device several times over but never more than
 * the largest job needs; a launch takes at most 65535 jobs (gridDim.y) */
constexpr size_t kMaxJobs = 65535;
dim3 move_grid(size_t n, uint64_t max_bytes)
{
    size_t blocks = (size_t)((max_bytes + (uint64_t)kThreads * 64 - 1) / ((uint64_t)kThreads * 64));
    size_t cap = (2048 + n - 1) / n;
    if (cap < 8) cap = 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks, (unsigned)n, 1);
}

} // namespace

hipError_t pl_launch_move(const PlMoveJob *d_jobs, size_t n, uint64_t max_bytes, hipStream_t stream)
{
    for (size_t first = 0; first < n; first += kMaxJobs) {
        const size_t m = n - first < kMaxJobs ? n - first : kMaxJobs;
        hipLaunchKernelGGL(pl_move, move_grid(m, max_bytes), dim3(kThreads), 0, stream, d_jobs + first);
    }
    return hipGetLastError();
}

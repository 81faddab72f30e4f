/*
 * pl_seg.hip -- kernels and launcher of the SEGMENT-PARALLEL row engine: one image spread over the whole MI355X.
 *
 * The algorithm, its proof obligation (the validation pass) and the kernel bodies live in pl_seg_core.h, which is also compiled
 * for the CPU by tests/c/seg_host.cpp; which launches an attempt is made of, their grids and workgroup sizes (their LDS bytes: pl_seg_lds.h), and what workgroup blockIdx.x of
 * each grid does live in pl_seg_launch.h, which the CPU harness runs too.  Here: the four gfx950 kernels of one row attempt, blockIdx.y = image of the batch,
 *
 *   seg_k_ctl     5 x 4 candidate workgroups (each a quarter of a candidate's decision tables) + 1 image-wide + W/256 commit workgroups
 *   seg_k_enum    3 x nseg x 2 workgroups of 512 lanes (a channel pair x 256 chain states; 1024 lanes = 4 channels for large batches) for the
 *                 filters that look at the left pixel, 2 x nseg/8 for none / up, 5 first-segment walkers; tables + pixel records in LDS
 *   seg_k_chain   5 x 4 workgroups, a row's dense transition tables (linked: an entry is the index of the next table's entry) and exit states in LDS (up to 149 KB of the CU's 160 KB)
 *   (seeded state sets only: seg_k_gather_seeded, 5 x 4 x nseg/4 workgroups of 256 lanes between the enumeration and the chain -- the chain's lookups by value)
 *   seg_k_replay  5 x ngrp workgroups: lane = (segment, quarter, channel), 8 steps each from the enumeration's checkpoints
 *   (the exact validation of every decision -- seg_post_body, 5 x 2 ngrp workgroups of 1024 lanes -- rides in seg_k_ctl's launch, one attempt behind)
 *
 * and no grid barrier anywhere: consecutive kernels on one stream are the grid-wide synchronisation (1.5-2 us on this machine
 * against 4-7 us for a hand-made in-kernel barrier across 8 XCDs, /opt/skills/guides/MI355X_MICROARCH.md), and every piece of
 * state is in device memory, so the host only enqueues attempts until the images report that they are finished.
 */
#include "pl_seg.h"

#include <atomic>

namespace {

__global__ void seg_k_resolve(const PlJob *jobs, SegJob *sj, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        sj[i].bpp = pl_job_bpp(jobs[sj[i].job_index]);
        sj[i].ctl[2].magic = 0u;          /* the image's first attempt (copy 0) finds no attempt behind it: no control block, */
        sj[i].acc[2].failmask = 0u;       /* ... no failed validation */
        for (int k = 0; k < 3; k++) { sj[i].v[k].magic = 0u; sj[i].v[k].finished = 0u; sj[i].v[k].ignore = 0u; sj[i].vfail[k] = 0u; }   /* (the same in the record's own copies) */
        sj[i].nbreak = 0u;
    }
}

/* The kernels of an attempt: each loads its image's record and hands its place in the grid to its dispatch function (pl_seg_launch.h), which knows what that
 * workgroup does.  (seg_k_ctl: SEG_EXPERIMENT_NO_VAL_CODE, a timing experiment, leaves the validation's code out of it and lifts its occupancy bound.)
 *
 * THE HEAD of each: the kernels' own arguments arrive in scalar registers at wave launch (the Makefile builds this file with kernel-argument preloading: no
 * load of the kernel-argument segment in front of the record's -- 0.2-0.4 us a kernel, profiles/seg_heads.txt), so no kernel here may use a hidden argument:
 * gridDim.x is the launcher's grid_x, passed by value where a dispatch function reads it.  The replay alone also requests its view and the record fields that its
 * dispatch and its first data request need in ONE burst of scalar loads in front of its first branch (pl_seg_launch.h: seg_view_of, seg_head_pin); what the body
 * reads late it reads from lines that this burst has brought into the scalar cache. */
#define SEG_GX_UNUSED 0u                  /* for the dispatch functions that ignore their gx */

#if SEG_EXPERIMENT_NO_VAL_CODE
#define SEG_CTL_BOUNDS __launch_bounds__(SEG_THREADS)
#else
#define SEG_CTL_BOUNDS __launch_bounds__(SEG_THREADS, 8)
#endif
template <int TPARTS>
__global__ SEG_CTL_BOUNDS void seg_k_ctl(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int k, unsigned nctl, unsigned max_ngrp)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_ctl<TPARTS>(j, sj + blockIdx.y, *P, k, nctl, max_ngrp, blockIdx.x, SEG_GX_UNUSED, seg_smem);
}

template <int NT>
__global__ __launch_bounds__(NT) void seg_k_enum(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par, unsigned max_nseg, unsigned grid_x)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_enum<NT>(j, sj + blockIdx.y, *P, par, max_nseg, blockIdx.x, grid_x, seg_smem);
}

template <int NT>
__global__ __launch_bounds__(NT) void seg_k_enum_seeded(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par, unsigned max_nseg)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_enum_seeded<NT>(j, sj + blockIdx.y, *P, par, max_nseg, blockIdx.x, SEG_GX_UNUSED, seg_smem);
}

/* (the second bound asks for 8 waves per SIMD: the body's 100 SGPRs held it at 7 -- three workgroups of 8 waves per CU where LDS and threads allow four; with 78 + spills to
 *  vector lanes a batch of more workgroups than slots gains: 96 frames of 1080p 312 -> 301 ms, 128: 403 -> 392; 16 ... 64 frames within +-0.7 %) */
template <int UNIT>
__global__ __launch_bounds__(SEG_UNT, 8) void seg_k_enum_unit(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par, unsigned perb, unsigned pers, int seeds)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_enum_unit<UNIT>(j, sj + blockIdx.y, *P, par, perb, pers, seeds, blockIdx.x, SEG_GX_UNUSED, seg_smem);
}

template <bool SEEDED, int CT, bool UNITS>
__global__ __launch_bounds__(CT) void seg_k_chain(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_chain<SEEDED, CT, UNITS>(j, sj + blockIdx.y, *P, par, blockIdx.x, SEG_GX_UNUSED, seg_smem);
}

template <int RNT>
__global__ __launch_bounds__(RNT) void seg_k_replay(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par, unsigned max_ngrp)
{
    extern __shared__ __align__(16) unsigned char seg_smem[];
    const SegJob j = sj[blockIdx.y];
#if defined(__HIP_DEVICE_COMPILE__)
    seg_head_pin(seg_view_words(sj + blockIdx.y, par), j.img, j.W, j.bpp, j.rowcopy, j.ctl, j.base, j.H0, j.acc, j.tables, j.rck, j.dnout, j.nseg, j.ngrp);
#endif
    seg_dispatch_replay<RNT>(j, sj + blockIdx.y, *P, par, max_ngrp, blockIdx.x, SEG_GX_UNUSED, seg_smem);
}

/* The ORDER of the kernels in the code object, pinned: the one-image kernels first, in the order round 4's library had them, the kernels of batches behind
 * them.  (Measured, profiles/r05_code_layout.txt: with the batch kernels emitted in between, the control kernel -- byte for byte the same instructions --
 * took 0.45 us longer per launch, the enumeration 0.5: the headline lost 3 %.) */
template __global__ void seg_k_ctl<SEG_TPARTS>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned);
template __global__ void seg_k_replay<SEG_REPLAY_NT>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned);
template __global__ void seg_k_chain<false, SEG_CHAIN_THREADS, false>(const SegJob *__restrict__, const SegParams *__restrict__, int);
template __global__ void seg_k_chain<true, SEG_CHAIN_THREADS, false>(const SegJob *__restrict__, const SegParams *__restrict__, int);
template __global__ void seg_k_enum_seeded<512>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned);
template __global__ void seg_k_enum_seeded<1024>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned);
template __global__ void seg_k_enum<512>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned);
template __global__ void seg_k_enum<1024>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned);
template __global__ void seg_k_ctl<SEG_TPARTS_BATCH>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned);
template __global__ void seg_k_enum_unit<SEG_UNIT>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned, int);
template __global__ void seg_k_chain<false, SEG_CHAIN_THREADS_UNIT, true>(const SegJob *__restrict__, const SegParams *__restrict__, int);
template __global__ void seg_k_replay<SEG_REPLAY_NT_BATCH>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned);
#if SEG_UNIT != 1
template __global__ void seg_k_enum_unit<1>(const SegJob *__restrict__, const SegParams *__restrict__, int, unsigned, unsigned, int);      /* (round 6; behind the pinned kernels) */
#endif

/* (seeded state sets; behind the pinned kernels: it joins the code object at its end) */
__global__ __launch_bounds__(SEG_GT) void seg_k_gather_seeded(const SegJob *__restrict__ sj, const SegParams *__restrict__ P, int par, unsigned nblk)
{
    const SegJob j = sj[blockIdx.y];
    seg_dispatch_gather(j, sj + blockIdx.y, *P, par, nblk, blockIdx.x, SEG_GX_UNUSED, nullptr);
}

/* the kernels of the engine whose dynamic LDS can exceed 64 KB: opted in per device (pl_lds_optin) */
hipError_t chain_attr()
{
    static std::atomic<unsigned> done_chain{ 0 }, done_ctl{ 0 };
    static std::atomic<unsigned> done_chain_s{ 0 };
    static std::atomic<unsigned> done_chain_u{ 0 };
    hipError_t e = pl_lds_optin((const void *)seg_k_chain<false, SEG_CHAIN_THREADS, false>, seg_lds_chain_bytes<true>(SEG_CHAIN_CAP + 1), done_chain);
    if (e == hipSuccess) e = pl_lds_optin((const void *)seg_k_chain<false, SEG_CHAIN_THREADS_UNIT, true>, seg_lds_chain_bytes<true>(SEG_CHAIN_CAP + 1), done_chain_u);
    if (e == hipSuccess) e = pl_lds_optin((const void *)seg_k_chain<true, SEG_CHAIN_THREADS, false>, seg_lds_chain_bytes<true>(SEG_CHAIN_CAP + 1), done_chain_s);
    static std::atomic<unsigned> done_ctl1{ 0 };
    if (e == hipSuccess && seg_lds_ctl_bytes<SEG_TPARTS>() > 65536) e = pl_lds_optin((const void *)seg_k_ctl<SEG_TPARTS>, seg_lds_ctl_bytes<SEG_TPARTS>(), done_ctl);
    if (e == hipSuccess && seg_lds_ctl_bytes<SEG_TPARTS_BATCH>() > 65536) e = pl_lds_optin((const void *)seg_k_ctl<SEG_TPARTS_BATCH>, seg_lds_ctl_bytes<SEG_TPARTS_BATCH>(), done_ctl1);
    return e;
}

} // namespace

#if SEG_EXPERIMENT_TAIL_PLACEMENT
/* MEASUREMENT BUILD only (tools/enum_tail_placement.py): the records of seg_enum_body_k's tail waves, copied to `out`; returns their words, 0 on an error */
extern "C" __attribute__((visibility("default"))) size_t pngloss_hip_debug_tail_placement(uint32_t *out, size_t words)
{
    const size_t n = sizeof(seg_tail_dbg) / sizeof(uint32_t);
    if (!out || words < n || hipDeviceSynchronize() != hipSuccess) return 0;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(seg_tail_dbg), sizeof(seg_tail_dbg)) == hipSuccess ? n : 0;
}
#endif

hipError_t pl_seg_launch_resolve(const PlJob *d_jobs, SegJob *d_sj, size_t n, hipStream_t stream)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(seg_k_resolve, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_jobs, d_sj, (unsigned)n);
    return hipGetLastError();
}

hipError_t pl_seg_launch_attempt(const PlSegBatch &b, int attempt, hipStream_t stream)
{
    if (!b.n) return hipSuccess;
    hipError_t e = chain_attr();
    if (e != hipSuccess) return e;
    const int par = attempt % 3;                               /* which copy of the control block / sums / histogram / prefix bumps the attempt writes */
    SegLaunch launches[SEG_MAX_LAUNCHES];
    const int nl = seg_attempt_launches(b.shape, launches);
    for (int i = 0; i < nl; i++) {
        const SegLaunch &L = launches[i];
        const dim3 grid(L.grid_x, (unsigned)b.n), block(L.threads);
#define SEG_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, grid, block, L.lds_bytes, stream, b.d_sj, b.d_params, par, ##__VA_ARGS__)
        switch (L.kernel) {
        case SEG_KERNEL_CTL: SEG_LAUNCH(seg_k_ctl<SEG_TPARTS>, L.a, L.b); break;
        case SEG_KERNEL_CTL_BATCH: SEG_LAUNCH(seg_k_ctl<SEG_TPARTS_BATCH>, L.a, L.b); break;
        case SEG_KERNEL_ENUM_512: SEG_LAUNCH(seg_k_enum<512>, L.a, L.grid_x); break;
        case SEG_KERNEL_ENUM_1024: SEG_LAUNCH(seg_k_enum<1024>, L.a, L.grid_x); break;
        case SEG_KERNEL_ENUM_SEEDED_512: SEG_LAUNCH(seg_k_enum_seeded<512>, L.a); break;
        case SEG_KERNEL_ENUM_SEEDED_1024: SEG_LAUNCH(seg_k_enum_seeded<1024>, L.a); break;
        case SEG_KERNEL_ENUM_UNIT: SEG_LAUNCH(seg_k_enum_unit<SEG_UNIT>, L.a, L.b, L.seeds); break;
        case SEG_KERNEL_ENUM_UNIT1: SEG_LAUNCH(seg_k_enum_unit<1>, L.a, L.b, L.seeds); break;
        case SEG_KERNEL_GATHER_SEEDED: SEG_LAUNCH(seg_k_gather_seeded, L.a); break;
        case SEG_KERNEL_CHAIN: SEG_LAUNCH((seg_k_chain<false, SEG_CHAIN_THREADS, false>)); break;
        case SEG_KERNEL_CHAIN_SEEDED: SEG_LAUNCH((seg_k_chain<true, SEG_CHAIN_THREADS, false>)); break;
        case SEG_KERNEL_CHAIN_UNIT: SEG_LAUNCH((seg_k_chain<false, SEG_CHAIN_THREADS_UNIT, true>)); break;
        case SEG_KERNEL_REPLAY: SEG_LAUNCH(seg_k_replay<SEG_REPLAY_NT>, L.a); break;
        case SEG_KERNEL_REPLAY_BATCH: SEG_LAUNCH(seg_k_replay<SEG_REPLAY_NT_BATCH>, L.a); break;
        case SEG_KERNEL_COUNT: break;
        }
#undef SEG_LAUNCH
    }
    return hipGetLastError();
}

/*
 * pl_seg.h -- host-side interface of the segment-parallel row engine (pl_seg.hip / pl_seg_core.h).  Internal.
 */
#ifndef PL_SEG_H
#define PL_SEG_H

#include "pl_device.h"
#include "pl_seg_launch.h"

/* (the per-image device workspace of the engine, beyond what PlJob already has, and which batches it takes: pl_plan.h) */

/* one launch group of a batch: its images' records and what its attempts look like (the SegShape of its PlSegGroupPlan) */
struct PlSegBatch {
    const SegJob *d_sj;       /* device: one per image */
    const SegParams *d_params;
    size_t n;
    SegShape shape;
};

/* fills sj[i].bpp from the class the prepare kernels detected */
hipError_t pl_seg_launch_resolve(const PlJob *d_jobs, SegJob *d_sj, size_t n, hipStream_t stream);
/* one attempt = [control + validation of the attempt before], enumerate, (seeded sets: gather,) chain, replay -- grids, workgroup sizes and LDS bytes: seg_attempt_launches,
 * pl_seg_launch.h (attempt: counted by the caller, any starting point that is a multiple of 3) */
hipError_t pl_seg_launch_attempt(const PlSegBatch &b, int attempt, hipStream_t stream);

#endif

/* pl_target_dev.h -- launcher of the batched move of pngloss_hip_optimize_batch_target (pl_target.hip).  Internal. */
#ifndef PL_TARGET_DEV_H
#define PL_TARGET_DEV_H

#include <hip/hip_runtime.h>

#include "pl_move_core.h"

/* n jobs in device memory, one launch (blockIdx.y = job); max_bytes: the largest `bytes` of them (sizes the grid).  n == 0: nothing is launched. */
hipError_t pl_launch_move(const PlMoveJob *d_jobs, size_t n, uint64_t max_bytes, hipStream_t stream);

#endif

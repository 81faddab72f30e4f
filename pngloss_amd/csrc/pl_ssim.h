/* pl_ssim.h -- device job of the structural similarity measurement (pl_ssim.hip).  Internal. */
#ifndef PL_SSIM_H
#define PL_SSIM_H

#include <hip/hip_runtime.h>

#include "pl_ssim_core.h"

/* One job = one image pair: the original, the result, their size, where the record goes */
struct PlSsimJob {
    const uint32_t *a;          /* device: width * height words of RGBA8, the original (the keep arena's copy; pngloss_hip_compare_batch_ssim: the caller's d_a) */
    const uint32_t *b;          /* device: the result (pngloss_hip_compare_batch_ssim: the caller's d_b) */
    uint32_t width, height;
    PlSsimRecord *record;       /* device, holding pls_record_begin(width, height) before pl_ssim is launched (pl_ssim_visible: pls_record_begin_visible()) */
};

/* max_tiles: the largest pls_geom(width, height).tiles of the n jobs (sizes the grid).  visible: measure over visible pixels (pl_ssim_core.h) */
hipError_t pl_launch_ssim(const PlSsimJob *d_jobs, size_t n, uint64_t max_tiles, hipStream_t stream, bool visible = false);

#endif

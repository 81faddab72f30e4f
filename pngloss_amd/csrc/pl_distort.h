/* pl_distort.h -- device job of the distortion measurement (pl_distort.hip).  Internal. */
#ifndef PL_DISTORT_H
#define PL_DISTORT_H

#include <hip/hip_runtime.h>

#include "pl_distort_core.h"

/* One job = one image: where its original is kept, where its pixels are, where its record goes */
struct PlDistortJob {
    uint32_t *keep;             /* device: `pixels` words of RGBA8 -- pl_keep writes them, pl_distort reads them (pngloss_hip_compare_batch: the caller's d_a) */
    const uint32_t *img;        /* device: the image itself: pl_keep reads the original, pl_distort the final pixels (pngloss_hip_compare_batch: the caller's d_b) */
    uint64_t pixels;
    PlDistortRecord *record;    /* device, zeroed before pl_distort is launched */
};

/* max_pixels: the largest `pixels` of the n jobs (sizes the grid).  visible: measure over visible pixels (pl_distort_core.h): record->pixels is then counted
 * by the kernel, from the zero the caller put there. */
hipError_t pl_launch_keep(const PlDistortJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream);
hipError_t pl_launch_distort(const PlDistortJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible = false);

#endif

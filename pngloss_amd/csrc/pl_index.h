/* pl_index.h -- device jobs of the indexed-colour write side (pl_index.hip).  Internal. */
#ifndef PL_INDEX_H
#define PL_INDEX_H

#include <hip/hip_runtime.h>

#include "pl_index_core.h"

/* One job = one image.  pl_index_count reads img / pixels and fills table / count; the two kernels behind it run on the eligible images only. */
struct PlIndexJob {
    const uint32_t *img;        /* device: width * height words of RGBA8, the optimised image */
    uint64_t pixels;
    uint32_t width, height;
    uint64_t *table;            /* device: PLI_SLOTS slots, all PLI_EMPTY before pl_index_count */
    uint32_t *count;            /* device: zero before pl_index_count; afterwards the insertions: the colours, exact up to 256, beyond it "more" */
    PliRecord *record;          /* device: zero before pl_index_palette */
    uint8_t *ids;               /* device: height filter type bytes, pl_index_rows writes 0 into each */
    uint8_t *rows;              /* device: height index rows, `pitch` bytes apart; pitch is a multiple of 4 and >= width */
    uint32_t pitch, reserved;
};

/* max_pixels / max_height: the largest of the n jobs (size the grids).  All asynchronous on `stream`. */
hipError_t pl_launch_index_count(const PlIndexJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream);
hipError_t pl_launch_index_palette(const PlIndexJob *d_jobs, size_t n, hipStream_t stream);
hipError_t pl_launch_index_rows(const PlIndexJob *d_jobs, size_t n, uint32_t max_height, hipStream_t stream);

#endif

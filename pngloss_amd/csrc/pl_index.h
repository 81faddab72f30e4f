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

/* Option "index_depth": one job = one eligible image with min_depth < 8, behind pl_index_rows.  pl_index_pack reads the 8-bit index rows and
 * writes the rows packed at `depth`; the jobs of one launch may differ in depth. */
struct PlPackJob {
    const uint8_t *rows8;       /* device: PlIndexJob::rows, 16-byte aligned, `pitch8` bytes apart (a multiple of 16, >= width) */
    uint8_t *ids;               /* device: height filter type bytes of the packed rows, pl_index_pack writes 0 into each */
    uint8_t *rows;              /* device: height packed rows, `pitch` bytes apart; pitch is a multiple of 4 and >= 4 * pli_packed_dwords(width, depth) */
    uint32_t width, height, pitch8, pitch;
    uint32_t depth, reserved;   /* 1, 2 or 4 */
};

static_assert(sizeof(PlIndexJob) == 72 && sizeof(PlPackJob) == 48, "the job records as tests/c/index_depth_host.cpp lays them out (it cannot include this header: no HIP runtime there)");

hipError_t pl_launch_index_pack(const PlPackJob *d_jobs, size_t n, uint32_t max_height, hipStream_t stream);

#endif

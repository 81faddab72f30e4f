/* pl_quant.h -- device jobs of the colour quantiser (pl_quant.hip).  Internal. */
#ifndef PL_QUANT_H
#define PL_QUANT_H

#include <hip/hip_runtime.h>

#include "pl_quant_core.h"
#include "pl_quant_measure_core.h"

/* One job = one image.  pl_quant_hist reads img / pixels and fills hist; the other kernels run on the images that are not exact only. */
struct PlQuantJob {
    const uint32_t *img;        /* device: `pixels` words of RGBA8, the input */
    uint32_t *out;              /* device: `pixels` words: the remap pass writes the quantised image here, beside the input */
    uint64_t pixels;
    uint32_t *hist;             /* device: PLQ_BINS counts, zero before pl_quant_hist */
    uint32_t *pal;              /* device: PLQ_MAX_COLORS words, the first `entries` of them the palette */
    uint64_t *acc;              /* device: PLQ_MAX_COLORS * PLQ_CELLS accumulators, zero before the first assign pass; pl_quant_update zeroes them again */
    uint32_t entries, reserved;
};

/* max_pixels: the largest `pixels` of the n jobs (sizes the grids).  All asynchronous on `stream`; no kernel waits for another workgroup.
 * visible: the kernels of the premultiplied space (include/pngloss_hip_quant_space.h) -- `pal` then holds premultiplied words, `out` gets straight ones */
hipError_t pl_launch_quant_hist(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible = false);
hipError_t pl_launch_quant_assign(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible = false);
hipError_t pl_launch_quant_remap(const PlQuantJob *d_jobs, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible = false);
/* the remap pass without its stores: the distortion record of (img, img remapped to the job's palette) added up in d_records[k] for job k; the
 * records are zero before the launch, and `pixels` of each is the caller's to write -- visible: the visible-mode record, `pixels` counted by the kernel */
hipError_t pl_launch_quant_measure(const PlQuantJob *d_jobs, PlDistortRecord *d_records, size_t n, uint64_t max_pixels, hipStream_t stream, bool visible = false);
hipError_t pl_launch_quant_update(const PlQuantJob *d_jobs, size_t n, hipStream_t stream);

#endif

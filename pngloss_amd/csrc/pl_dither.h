/* pl_dither.h -- device job of the quantiser's error diffusion (pl_dither.hip).  Internal. */
#ifndef PL_DITHER_H
#define PL_DITHER_H

#include <hip/hip_runtime.h>

#include "pl_dither_core.h"

/* One job = one working image (not exact, with pixels): the remap step of the quantiser with Floyd-Steinberg error diffusion. */
struct PlDitherJob {
    const uint32_t *img;        /* device: width * height words of RGBA8, the input */
    uint32_t *out;              /* device: width * height words: the dithered image, beside the input */
    const uint32_t *pal;        /* device: the first `entries` words the final palette */
    PlfErr *line;               /* device: `width` entries: the errors of a band's last row, for the band below */
    uint32_t width, height, entries, reserved;
};

/* One workgroup per job.  Asynchronous on `stream`; no kernel waits for another workgroup.  visible: the rule of the premultiplied space
 * (include/pngloss_hip_quant_space.h) -- `pal` holds premultiplied words, `out` gets straight ones */
hipError_t pl_launch_dither(const PlDitherJob *d_jobs, size_t n, hipStream_t stream, bool visible = false);

#endif

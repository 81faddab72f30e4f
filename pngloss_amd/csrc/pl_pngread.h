/* pl_pngread.h -- device job of the PNG read side (pl_pngread.hip).  Internal. */
#ifndef PL_PNGREAD_H
#define PL_PNGREAD_H

#include <hip/hip_runtime.h>

#include "pl_pngread_core.h"

/* One job = one filtered image on the band wavefront: a whole non-interlaced file, or one non-empty Adam7 pass of an interlaced file */
struct PrJob {
    const uint8_t *raw;     /* device: height * (1 + rowbytes) inflated bytes, filter type first (a pass: its part of the file's bytes) */
    uint32_t *rgba;         /* device: the file's RGBA8 */
    uint8_t *lastrow;       /* device scratch: one row of `lastpitch` bytes per band of PR_ROWS rows (the band's last row, for the band below) */
    uint32_t *progress;     /* device, zeroed before the launch: per band, the number of blocks whose last row is in `lastrow` */
    uint32_t lastpitch, nbands;
    int32_t *status;        /* device: 0 or 25, one word per file (the passes of a file share it) */
    /* placement: pixel (x, y) of the job is pixel (ox + x * sx, oy + y * sy) of the file, stored at rgba[(oy + y * sy) * pitch + ox + x * sx];
     * a non-interlaced file is (0, 0, 1, 1, width) */
    uint32_t ox, oy, sx, sy, pitch;
    PrFormat F;             /* the file's format with the job's width, height and rowbytes (a pass: its own) */
};

hipError_t pl_launch_png_decode(const PrJob *d_jobs, size_t n, uint32_t max_bands, hipStream_t stream);

#endif

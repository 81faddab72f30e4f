/*
 * pngloss_hip_quant.h -- the colour-quantiser extension of the C ABI of libpngloss_hip.so (include/pngloss_hip.h): two calls that make RGBA8 images
 * have at most N colours, on the device, so that the option "indexed" (pngloss_hip_indexed.h) finds a palette.  Plain C; includes pngloss_hip.h.
 */
#ifndef PNGLOSS_HIP_QUANT_H
#define PNGLOSS_HIP_QUANT_H

#include "pngloss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Colour quantisation (no reference equivalent: the reference tool never reduces the number of colours, and says of itself that it "does not do a
 * good job on paletted images or images with large areas of flat color").  These are CALLS, not an option: the results of every other call depend on
 * no option, as before.  Everything is an integer, so the device's answer is defined bit for bit.  A pixel is its RGBA8 word, channels R, G, B, A
 * in that order; all four channels weigh the same (the search on alpha-premultiplied
 * pixels instead, where what transparency hides costs nothing: pngloss_hip_quant_space.h).  Dithering: pngloss_hip_dither.h.
 *   exact        An image with at most max_colors distinct words comes back unchanged: exact = 1, palette = its colours ascending by the word read as a
 *                little-endian uint32 (the palette order of pngloss_hip_indexed.h).  An image without pixels is exact with 0 entries.
 *   histogram    bin(p) = (R>>4) | (G>>4)<<4 | (B>>4)<<8 | (A>>4)<<12: 65 536 bins; a bin's coordinate on a channel is that channel's 4-bit field.
 *   median cut   Over the non-empty bins.  A box is a list of bins; its range on a channel is the largest minus the smallest coordinate.  Start with
 *                one box of every non-empty bin, ascending.  While there are fewer than max_colors boxes and some box has a non-zero range, split the
 *                box with the largest pixel count among those with a non-zero range (tie: the first in the list) on its channel of largest range (tie:
 *                the lowest channel): with lo, hi that channel's smallest and largest coordinate in the box, the cut t is the smallest value in
 *                lo .. hi-1 for which twice the pixels with coordinate <= t is at least the box's pixel count, or hi-1 if there is none; the box is
 *                replaced in place by (coordinate <= t), then (coordinate > t).  A box's colour is per channel (2*S + P) / (2*P), rounded down, where
 *                S = the sum over its bins of count * (16 * coordinate + 8) and P = its pixel count.  That is the initial palette: 1 .. max_colors entries.
 *   refinement   `rounds` times: every pixel goes to the entry with the smallest squared distance over the four channels (tie: the lowest entry); an
 *                entry that got pixels becomes (2*sum + count) / (2*count) per channel, rounded down; one that got none stays as it is.
 *   remap        every pixel becomes the word of its nearest entry of the final palette (same rule).  Entries may repeat or go unused: the palette
 *                that is REPORTED is the distinct words of the remapped image, ascending -- what the option "indexed" will find in it. */
typedef struct {
    uint32_t max_colors;       /* N, 2 .. 256 */
    uint32_t rounds;           /* R, 0 .. 64; PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS is what the command line tool uses */
} pngloss_hip_quant_params;

#define PNGLOSS_HIP_QUANT_DEFAULT_ROUNDS 8

/* What happened to one image */
typedef struct {
    int32_t  status;           /* 0 */
    uint32_t colors_in;        /* distinct colours of the input; 257 = "more than 256"; 0 for an image without pixels */
    uint32_t entries;          /* distinct colours of the image as it is now: at most max_colors */
    uint32_t exact;            /* 1: the input had at most max_colors colours and was not changed */
    uint32_t palette[256];     /* the first `entries`: the colours of the image as it is now, ascending; the others 0 */
    pngloss_hip_distortion distortion;   /* the image as it is now against the input, over all pixels (pngloss_hip_compare_batch's record) */
} pngloss_hip_quant_report;

/* Quantise n device-resident images (d_rgba: width * height RGBA8 words; d_row_filters is ignored) in place.  SYNCHRONOUS: the median cut runs on
 * the host, so the call waits for the device twice -- once behind the histograms, once at the end -- and has finished when it returns; everything
 * it enqueues goes to `stream`.  Its workspace (per image about 300 KiB of tables and width * height * 4 bytes for the result, which lies beside
 * the input until its distortion record is taken) is allocated before anything is enqueued: if it cannot be had the call returns
 * PNGLOSS_OUT_OF_MEMORY_ERROR and nothing has run.  PNGLOSS_INVALID_ARGUMENT, before any device work: ctx, params or (with n > 0) images or reports
 * NULL, max_colors outside 2 .. 256, rounds above 64, an image with pixels and no d_rgba or with 2^32 pixels or more (a histogram bin is a 32-bit count
 * and may take every pixel), a batch in flight on the context.  The "last batch" of the context (pngloss_hip_last_*) is not touched. */
int pngloss_hip_quantize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params *params,
                               pngloss_hip_quant_report *reports, void *stream);

/* The host form over every context of `multi`: images[i].rgba is quantised where it lies in the caller's memory (row_filters is ignored), the images
 * dealt out like those of pngloss_hip_multi_optimize_batch_host, reports[i] is images[i]'s whichever context it went to.  The same argument checks;
 * the code of a call whose contexts answered differently is folded as there.  pngloss_hip_multi_last_* have nothing to index behind this call. */
int pngloss_hip_multi_quantize_batch_host(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                          const pngloss_hip_quant_params *params, pngloss_hip_quant_report *reports);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_QUANT_H */

/*
 * pngloss_hip_dither.h -- the dithering extension of the colour quantiser of libpngloss_hip.so (include/pngloss_hip_quant.h): the two calls of that
 * header again, with a parameter record that can ask for Floyd-Steinberg error diffusion in the remap step.  Plain C; includes pngloss_hip_quant.h.
 */
#ifndef PNGLOSS_HIP_DITHER_H
#define PNGLOSS_HIP_DITHER_H

#include "pngloss_hip_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PNGLOSS_HIP_DITHER_NONE 0
#define PNGLOSS_HIP_DITHER_FLOYD_STEINBERG 1

/* Dithering replaces only the last step of pngloss_hip_quant.h, the remap.  The exact test, the histogram, the median cut and the `rounds` refinement
 * rounds are as stated there; refinement stays undithered.  An exact image (at most max_colors colours) comes back unchanged and is never dithered.
 * Everything is an integer, so the device's answer is defined bit for bit.  For a working image of width W and height H with the final palette
 * pal[0 .. E):
 *   order        The pixels are visited in raster order: y ascending, then x ascending.  There is no serpentine.
 *   error        e_c(y, x) is the signed error of channel c at a visited pixel; it is 0 for every position outside the image.
 *   gather       S_c = 7 * e_c(y, x-1) + 1 * e_c(y-1, x-1) + 5 * e_c(y-1, x) + 3 * e_c(y-1, x+1)
 *                a_c = p_c(y, x) + floor((S_c + 8) / 16)                    (an arithmetic shift by 4)
 *                v_c = min(255, max(0, a_c)), and v is the RGBA8 word of the four v_c
 *   search       k = the entry nearest to v by the rule of pngloss_hip_quant.h: the smallest squared distance over the four channels, the lowest
 *                index among equals
 *   output       the pixel becomes pal[k], and e_c(y, x) = v_c - pal[k]_c
 * All four channels diffuse alike, alpha included.  |e_c| <= 255, |S_c| <= 4080, -255 <= a_c <= 510.  This is the gather form, one division per
 * pixel and channel: no error is lost to rounding per term.
 * The reported palette, entries, colors_in, exact and the distortion record are produced as pngloss_hip_quant.h says, from the dithered image:
 * `entries` may come out larger than without dithering -- entries that the nearest-entry remap left unused get used -- and is still at most max_colors.
 * A single image is dithered by one workgroup, on one compute unit: error diffusion is a serial chain, of which min(H, W/2) pixels are independent at
 * any time.  A batch spreads over the device, an image per workgroup. */
typedef struct {
    uint32_t max_colors;       /* N, 2 .. 256 */
    uint32_t rounds;           /* R, 0 .. 64 */
    uint32_t dither;           /* PNGLOSS_HIP_DITHER_NONE = 0, PNGLOSS_HIP_DITHER_FLOYD_STEINBERG = 1 */
    uint32_t reserved;         /* 0 */
} pngloss_hip_quant_params2;

/* pngloss_hip_quantize_batch with a pngloss_hip_quant_params2: the same contract -- synchronous, two waits, the workspace (with dither = 1 another
 * 8 * width bytes per image) grown before anything is enqueued, the same refusals, the last batch untouched.  Further refusals, before any device work:
 * dither above 1 or reserved not 0 returns PNGLOSS_INVALID_ARGUMENT.  With dither = 0 the call does bit for bit what pngloss_hip_quantize_batch does. */
int pngloss_hip_quantize_batch2(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
                                pngloss_hip_quant_report *reports, void *stream);

/* pngloss_hip_multi_quantize_batch_host with a pngloss_hip_quant_params2, in the same way. */
int pngloss_hip_multi_quantize_batch_host2(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                           const pngloss_hip_quant_params2 *params, pngloss_hip_quant_report *reports);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_DITHER_H */

/*
 * pngloss_hip_quant_space.h -- the colour quantiser of libpngloss_hip.so (include/pngloss_hip_quant.h, pngloss_hip_dither.h,
 * pngloss_hip_quant_target.h) with the space its palette search runs in: the RGBA8 words as they are, or the alpha-premultiplied words, where what
 * a viewer cannot see cannot cost anything.  Plain C; includes pngloss_hip_quant_target.h.
 */
#ifndef PNGLOSS_HIP_QUANT_SPACE_H
#define PNGLOSS_HIP_QUANT_SPACE_H

#include "pngloss_hip_quant_target.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PNGLOSS_HIP_QUANT_SPACE_RGBA    0
#define PNGLOSS_HIP_QUANT_SPACE_VISIBLE 1

/* Definitions (all integers).  Space 0 is pngloss_hip_quant.h as it stands: alpha is a fourth channel, all four weigh the same.  Space 1:
 *   pm(p)        pngloss_hip.h's ("Measuring over visible pixels"): alpha stays, each of R, G, B becomes (c * A + 127) / 255, rounded down.
 *   straight(e)  for a palette entry e = (r', g', b', a): a == 0 gives the word 0; otherwise each of R, G, B becomes
 *                min(255, (c' * 255 + a / 2) / a), rounded down, and alpha stays.
 *   not exact    The histogram, the median cut, the refinement rounds and the nearest-entry rule of pngloss_hip_quant.h are applied to the words
 *                pm(p) instead of p; palette entries are premultiplied words.  Remap: pixel p becomes straight(pal[k]), k the entry nearest to pm(p).
 *                So a fully transparent pixel comes back as the word 0 whatever RGBA it hid, and all of them share one bin, one box and one entry.
 *   exact        as in space 0, decided on the straight words: an image with at most max_colors distinct words comes back unchanged, never dithered.
 *   palette, entries, colors_in   as in space 0: the distinct words of the image as it is now.
 *   distortion   the VISIBLE-mode record of (input, output): the sums over pm(input), pm(output), `pixels` the count of pixels whose alpha is
 *                non-zero in either -- what pngloss_hip_compare_batch reports with the option "measure" at "visible".
 *   dithering    pngloss_hip_dither.h's rule with p_c the channels of pm(pixel), the search over the premultiplied entries, the pixel becoming
 *                straight(pal[k]) and e_c = v_c - pal[k]_c in premultiplied units; and a pixel with alpha 0 takes no error in: for it S_c counts
 *                as 0, so v = 0 (diffusion does not sprinkle faint pixels into a sprite's transparent surround).  It still passes its own error
 *                0 - pal[k]_c on.  |e_c| <= 255 and |S_c| <= 4080 hold as they are.
 *   colour-count search   pngloss_hip_quant_target.h's procedure; a probe's record is the visible-mode record; a probe whose record has
 *                pixels == 0 is accepted (nothing to see in either image; pngloss_hip_psnr_db is NaN there); for an exact probe
 *                probe_distortion.pixels equals quant.distortion.pixels.
 * Two facts.  pm(straight(e)) == e for every entry with r', g', b' <= a, and every entry the median cut or a round makes of premultiplied pixels has
 * r', g', b' <= a: the record is that of the words the search compared.  straight's min(255, ...) makes it total all the same.
 * Space 1 is no guarantee per image: another first bin sends the median cut elsewhere, and an image with binary alpha can lose a fraction of a dB.
 * Not built: a perceptual (gamma, channel-weighted) distance, an alpha-aware exact test, SSIM targets for the colour count. */
typedef struct {
    uint32_t max_colors;       /* N, 2 .. 256 */
    uint32_t rounds;           /* R, 0 .. 64 */
    uint32_t dither;           /* PNGLOSS_HIP_DITHER_NONE = 0, PNGLOSS_HIP_DITHER_FLOYD_STEINBERG = 1 */
    uint32_t space;            /* PNGLOSS_HIP_QUANT_SPACE_RGBA = 0, PNGLOSS_HIP_QUANT_SPACE_VISIBLE = 1 */
} pngloss_hip_quant_params3;   /* (pngloss_hip_quant_params2's layout, `reserved` named) */

/* pngloss_hip_quantize_batch2 with a pngloss_hip_quant_params3: the same contract, the same workspace, the same refusals.  One more refusal, before
 * any device work: space above 1 returns PNGLOSS_INVALID_ARGUMENT.  With space = 0 the call does bit for bit what pngloss_hip_quantize_batch2 does. */
int pngloss_hip_quantize_batch3(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params3 *params,
                                pngloss_hip_quant_report *reports, void *stream);

/* pngloss_hip_multi_quantize_batch_host2 with a pngloss_hip_quant_params3, in the same way. */
int pngloss_hip_multi_quantize_batch_host3(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                           const pngloss_hip_quant_params3 *params, pngloss_hip_quant_report *reports);

/* pngloss_hip_quantize_batch_target and its host form with a pngloss_hip_quant_params3, in the same way. */
int pngloss_hip_quantize_batch_target3(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params3 *params,
                                       const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream);
int pngloss_hip_multi_quantize_batch_host_target3(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                                  const pngloss_hip_quant_params3 *params, const pngloss_hip_quant_target *target,
                                                  pngloss_hip_quant_target_report *reports);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_QUANT_SPACE_H */

/*
 * pngloss_hip_quant_target.h -- the colour quantiser of libpngloss_hip.so (include/pngloss_hip_quant.h, pngloss_hip_dither.h) with the number of
 * colours found per image from a distortion target: the fewest colours, by the procedure below, whose quantisation still meets a PSNR or a largest
 * channel error.  Plain C; includes pngloss_hip_dither.h.
 */
#ifndef PNGLOSS_HIP_QUANT_TARGET_H
#define PNGLOSS_HIP_QUANT_TARGET_H

#include "pngloss_hip_dither.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Definitions.  M = params->max_colors; `rounds` and `dither` are the call's.
 *   probe        "Probe image i at N": what pngloss_hip_quantize_batch2 with max_colors = N and the call's rounds and dither does to the ORIGINAL
 *                image, and the pngloss_hip_distortion record of (original, result) over all pixels -- the record that call reports.
 *   acceptance   A probe is accepted when both hold: min_psnr_db == 0 or pngloss_hip_psnr_db(&record, 0xF) >= min_psnr_db; max_abs_error == 0 or the
 *                largest record.max_abs[c] is <= max_abs_error.
 *   no device work   An image without pixels is accepted.  A probe at N >= colors_in is exact: its record is all zero apart from `pixels`, its PSNR
 *                is +inf, and it is accepted with no device work.
 *   measure      The option "measure" is ignored: the quantiser's records are over all pixels.
 *   the chosen N PSNR is not monotone in N (one more colour can lower it), so the chosen N is what this procedure gives and not "the smallest N
 *                that passes":
 *                  1. probe M.  Refused: colors = M, reached = 0, and the image keeps the result at M
 *                  2. otherwise lo = 1, hi = M; N = 1 counts as refused without a probe
 *                  3. while hi - lo > 1: probe mid = (lo + hi) / 2, rounded down; accepted: hi = mid, otherwise lo = mid
 *                  4. colors = hi, reached = 1
 *                At most 1 + ceil(log2(M - 1)) probes: 9 for M = 256, 1 for M = 2.
 * The image is left exactly as pngloss_hip_quantize_batch2 at max_colors = colors leaves it. */
typedef struct {
    double   min_psnr_db;      /* 0 = no condition; +inf = only exact results pass; NaN or < 0 is invalid */
    uint32_t max_abs_error;    /* 0 = no condition; 1 .. 255; above 255 is invalid */
    uint32_t reserved;         /* 0 */
} pngloss_hip_quant_target;

#define PNGLOSS_HIP_QUANT_TARGET_MAX_PROBES 12

/* What the search did to one image */
typedef struct {
    uint32_t colors;           /* the chosen N */
    uint32_t reached;          /* 1: the target was met; 0: even M was refused */
    uint32_t probes;           /* number of probes */
    uint32_t accepted_mask;    /* bit k set = probe k was accepted */
    uint32_t probed[PNGLOSS_HIP_QUANT_TARGET_MAX_PROBES];   /* the N of probe k; the rest 0 */
    pngloss_hip_distortion probe_distortion;   /* the record the probe at `colors` took */
    pngloss_hip_quant_report quant;            /* what pngloss_hip_quantize_batch2 at max_colors = colors reports for this image, field for field */
} pngloss_hip_quant_target_report;

/* pngloss_hip_quantize_batch2 with the colour count searched per image.  SYNCHRONOUS: one wait behind the colour counts and the histograms (taken
 * once per call; the histograms stay on the host), one per round of probes -- all images still searching share a round's launches, each at its own
 * N -- and one at the end.  The argument checks of pngloss_hip_quantize_batch2, and PNGLOSS_INVALID_ARGUMENT for a NULL or invalid target or one with
 * neither condition (every probe would pass); all of them before any device work.  The workspace is grown before anything is enqueued: if it cannot
 * be had the call returns PNGLOSS_OUT_OF_MEMORY_ERROR and nothing has run.  The "last batch" of the context is not touched. */
int pngloss_hip_quantize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params2 *params,
                                      const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream);

/* The host form over every context of `multi`, dealt out like pngloss_hip_multi_quantize_batch_host2. */
int pngloss_hip_multi_quantize_batch_host_target(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                                 const pngloss_hip_quant_params2 *params, const pngloss_hip_quant_target *target,
                                                 pngloss_hip_quant_target_report *reports);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_QUANT_TARGET_H */

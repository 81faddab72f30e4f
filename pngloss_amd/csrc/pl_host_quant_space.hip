/*
 * pl_host_quant_space.hip -- the quantiser's entry points that name the space the palette search runs in (include/pngloss_hip_quant_space.h;
 * pl_host_ctx.h has the map of the host files).  A pngloss_hip_quant_params3 is a pngloss_hip_quant_params2 whose last word is the space: each entry
 * point checks that word, hands the rest on as the older record -- so every older refusal is made by the older check, with the older code -- and
 * calls what the older entry points call (pl_host_quant.hip, pl_host_quant_target.hip).  No device work here.
 */
#include "pl_host_ctx.h"

static_assert(sizeof(pngloss_hip_quant_params3) == sizeof(pngloss_hip_quant_params2) && offsetof(pngloss_hip_quant_params3, space) == offsetof(pngloss_hip_quant_params2, reserved) &&
              offsetof(pngloss_hip_quant_params3, dither) == offsetof(pngloss_hip_quant_params2, dither), "pngloss_hip_quant_params3 is pngloss_hip_quant_params2 with `reserved` named");

namespace {

/* The older record of a call, or nullptr for one the older check is to refuse as it refuses a missing record: no record, or a space that is none */
const pngloss_hip_quant_params2 *narrow(const pngloss_hip_quant_params3 *params, pngloss_hip_quant_params2 &older)
{
    if (!params || params->space > PNGLOSS_HIP_QUANT_SPACE_VISIBLE) return nullptr;
    older = pngloss_hip_quant_params2{ params->max_colors, params->rounds, params->dither, 0 };
    return &older;
}
uint32_t space_of(const pngloss_hip_quant_params3 *params) { return params ? params->space : PNGLOSS_HIP_QUANT_SPACE_RGBA; }

} // namespace

extern "C" {

int pngloss_hip_quantize_batch3(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params3 *params,
                                pngloss_hip_quant_report *reports, void *stream)
{
    pngloss_hip_quant_params2 older;
    return quantize_batch(ctx, images, n, narrow(params, older), space_of(params), reports, stream);
}

int pngloss_hip_multi_quantize_batch_host3(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params3 *params,
                                           pngloss_hip_quant_report *reports)
{
    pngloss_hip_quant_params2 older;
    return multi_quantize_batch_host(m, images, n, narrow(params, older), space_of(params), reports);
}

int pngloss_hip_quantize_batch_target3(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n, const pngloss_hip_quant_params3 *params,
                                       const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports, void *stream)
{
    pngloss_hip_quant_params2 older;
    return quantize_batch_target(ctx, images, n, narrow(params, older), space_of(params), target, reports, stream);
}

int pngloss_hip_multi_quantize_batch_host_target3(pngloss_hip_multi *m, const pngloss_hip_host_image *images, size_t n, const pngloss_hip_quant_params3 *params,
                                                  const pngloss_hip_quant_target *target, pngloss_hip_quant_target_report *reports)
{
    pngloss_hip_quant_params2 older;
    return multi_quantize_batch_host_target(m, images, n, narrow(params, older), space_of(params), target, reports);
}

} /* extern "C" */

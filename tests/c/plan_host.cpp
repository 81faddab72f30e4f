/*
 * plan_host.cpp -- TEST INFRASTRUCTURE: the batch plan of the library (pngloss_amd/csrc/pl_plan.h, the header pl_host.hip carries out) behind a
 * thin C ABI, so that the CPU suite pins every decision the library makes about a batch without a GPU (tests/test_plan_host.py).
 *
 *   plan_host_run(w, h, n, strength, bleed, engine, knobs[16], scales[3], out[16], on_seg[n], seg_list[n], groups[8 * 12])
 *   plan_host_enum_kind(segs, k, strength, bleed, seg_unit, seg_seeds, seg_seeds1)   -> PlEnumKind, or -1 if the engine cannot take the pair
 *   plan_host_seed_n(strength, bleed)                                                -> SegParams::seed_n (-1: no parameters for the pair)
 *   plan_host_parse_option(name)                                                     -> PlEnginePin, or -1 (pngloss_hip_set_option refuses it)
 *   plan_host_window(pixels, n, split, no_split, deflate, peers, first[9])           -> chunks K; first[0 .. K]
 */
#include "../../pngloss_amd/csrc/pl_plan.h"

#include <cstdint>

extern "C" {

/* knobs: [0] forced_filter  [1] rows_fit  [2] sync_call  [3] three_groups_ok  [4] opt_launch_groups  [5] stream_wait_used
 *        [6] seg_groups  [7] seg_unit  [8] tparts  [9] enum_nt  [10] kin  [11] seg_seeds  [12] seg_seeds1  [13] seed_kin  [14] force_careful  [15] segprof
 * scales: cus, seg, wg.  engine: the value of $PNGLOSS_HIP_ENGINE (NULL: unset).
 * out: [0] use_rows  [1] seg_costed  [2] seg_pin_unmet  [3] engine_mode  [4] kind  [5] ngroups  [6] unit  [7] tparts  [8] seed_kin  [9] kin
 *      [10] max_attempts  [11] images on the segment engine  [12] engine_flags  [13] seeded  [14] seed_n
 * groups[12 g + ..]: first, n, max_nseg, max_ngrp, max_ncommit, enum_nt, tparts, unit, seeds, small_ok, seeded, 0 */
void plan_host_run(const uint32_t *w, const uint32_t *h, size_t n, unsigned strength, long bleed, const char *engine, const int32_t *knobs,
                   const double *scales, int64_t *out, uint8_t *on_seg, uint32_t *seg_list, int64_t *groups)
{
    PlPlanInput in;
    in.width.assign(w, w + n);
    in.height.assign(h, h + n);
    in.strength = strength;
    in.bleed = bleed;
    in.pin = pl_engine_pin_of_env(engine);
    in.forced_filter = knobs[0];
    in.rows_fit = knobs[1] != 0;
    in.sync_call = knobs[2] != 0;
    in.three_groups_ok = knobs[3] != 0;
    in.opt_launch_groups = knobs[4];
    in.stream_wait_used = knobs[5] != 0;
    PlHooks &hk = in.hooks;
    hk.seg_groups = knobs[6]; hk.seg_unit = knobs[7]; hk.tparts = knobs[8]; hk.enum_nt = knobs[9]; hk.kin = knobs[10];
    hk.seg_seeds = knobs[11]; hk.seg_seeds1 = knobs[12]; hk.seed_kin = knobs[13]; hk.force_careful = knobs[14] != 0; hk.segprof = knobs[15] != 0;
    in.cus = scales[0]; in.seg_scale = scales[1]; in.wg_scale = scales[2];
    const PlPlan p = pl_plan_batch(in);
    out[0] = p.use_rows; out[1] = p.seg_costed; out[2] = p.seg_pin_unmet; out[3] = p.engine_mode; out[4] = (int64_t)p.kind; out[5] = p.ngroups;
    out[6] = p.params.unit; out[7] = p.params.tparts; out[8] = p.params.seed_kin; out[9] = p.params.kin; out[10] = p.max_attempts;
    out[11] = (int64_t)p.seg_list.size(); out[12] = p.params.engine_flags; out[13] = p.params.seeded; out[14] = p.params.seed_n;
    for (size_t i = 0; i < n; i++) on_seg[i] = p.on_seg[i];
    for (size_t i = 0; i < p.seg_list.size(); i++) seg_list[i] = p.seg_list[i];
    for (int g = 0; g < p.ngroups; g++) {
        const PlSegGroupPlan &b = p.group[g];
        int64_t *o = groups + 12 * g;
        o[0] = (int64_t)p.gfirst[g]; o[1] = (int64_t)b.n; o[2] = b.max_nseg; o[3] = b.max_ngrp; o[4] = b.max_ncommit; o[5] = b.enum_nt;
        o[6] = b.tparts; o[7] = b.unit; o[8] = b.seeds; o[9] = b.small_ok; o[10] = b.seeded; o[11] = 0;
    }
}

int plan_host_enum_kind(size_t segs, size_t k, unsigned strength, long bleed, int seg_unit, int seg_seeds, int seg_seeds1)
{
    SegParams P;
    if (!seg_build_params(P, (int)strength, (int)bleed)) return -1;
    return (int)pl_enum_kind(segs, k, P, seg_unit, seg_seeds, seg_seeds1);
}

int plan_host_seed_n(unsigned strength, long bleed)
{
    SegParams P;
    return seg_build_params(P, (int)strength, (int)bleed) ? P.seed_n : -1;
}

int plan_host_parse_option(const char *name)
{
    PlEnginePin p;
    return pl_engine_pin_parse(name, &p) ? (int)p : -1;
}

size_t plan_host_window(const uint64_t *pixels, size_t n, int split, int no_split, int deflate, size_t peers, size_t *first)
{
    PlHooks hk;
    hk.split = split;
    hk.no_split = no_split != 0;
    size_t K = pl_host_window_chunks(n, hk, deflate != 0);
    if (K > 1) K = std::min(K, peers + 1);
    if (K <= 1) { first[0] = 0; first[1] = n; return 1; }
    const std::vector<size_t> f = pl_host_window_cut(std::vector<uint64_t>(pixels, pixels + n), K);
    for (size_t c = 0; c <= K; c++) first[c] = f[c];
    return K;
}

} /* extern "C" */

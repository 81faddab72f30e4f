/*
 * pl_colors.h -- the decisions of pngloss_hip_quantize_batch_target: a colour count per image, found from a distortion target
 * (include/pngloss_hip_quant_target.h states the rule for callers).  No reference equivalent.
 *
 * Plain C++ without HIP types, like pl_target.h and pl_size.h: whether a target is valid, whether a probe is accepted, which N an image probes next
 * and which one it ends with, which probes need no device work, and who takes part in a round -- so that tests/c/colors_host.cpp drives it on the
 * CPU.  pl_host_quant_target.hip does what it says.
 *
 * The rule, per image.  PSNR is not monotone in N, so the result is defined by this procedure and not by "the smallest N that passes":
 *   1. probe M = max_colors; refused: the chosen N is M, the target is not reached
 *   2. else lo = 1, hi = M (N = 1 counts as refused without a probe)
 *   3. while hi - lo > 1: probe mid = (lo + hi) / 2; accepted: hi = mid, else lo = mid
 *   4. the chosen N is hi
 * At most 1 + ceil(log2(M - 1)) probes, 1 for M = 2.
 */
#ifndef PL_COLORS_H
#define PL_COLORS_H

#include "../../include/pngloss_hip_quant_target.h"
#include "pl_distort_core.h"

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

constexpr uint32_t PLC_MAX_PROBES = PNGLOSS_HIP_QUANT_TARGET_MAX_PROBES;

/* PNGLOSS_SUCCESS, or PNGLOSS_INVALID_ARGUMENT for a target the header rules out */
inline int pl_colors_target_check(const pngloss_hip_quant_target *t)
{
    if (!t) return PNGLOSS_INVALID_ARGUMENT;
    if (t->min_psnr_db != t->min_psnr_db || t->min_psnr_db < 0.0) return PNGLOSS_INVALID_ARGUMENT;      /* NaN, negative */
    if (t->max_abs_error > 255u || t->reserved) return PNGLOSS_INVALID_ARGUMENT;
    if (t->min_psnr_db == 0.0 && !t->max_abs_error) return PNGLOSS_INVALID_ARGUMENT;                    /* neither condition: every probe would pass */
    return PNGLOSS_SUCCESS;
}

/* Is a probe accepted: `rec` is the probed result against the original over all pixels and all four channels */
inline bool pl_colors_accept(const pngloss_hip_quant_target &t, const PlDistortRecord &rec)
{
    if (!rec.pixels) return true;                                 /* an image without pixels */
    if (t.min_psnr_db != 0.0 && !(pld_psnr_db(rec.pixels, rec.sq_err, 0xFu) >= t.min_psnr_db)) return false;
    if (t.max_abs_error) {
        uint32_t largest = 0;
        for (int c = 0; c < 4; c++)
            if (rec.max_abs[c] > largest) largest = rec.max_abs[c];
        if (largest > t.max_abs_error) return false;
    }
    return true;
}

/* The search of one image.  While !done, `next` is the N to probe; pl_colors_step takes that probe's verdict. */
struct PlColorsSearch {
    uint32_t lo = 1, hi = 0;
    uint32_t next = 0;
    uint32_t probes = 0;
    uint32_t chosen = 0;
    uint32_t accepted_mask = 0;
    uint32_t probed[PLC_MAX_PROBES] = {};
    bool first = true, done = false;
    bool reached = false;
};

/* the most probes a search up to M can take: 1 + ceil(log2(M - 1)) */
inline uint32_t pl_colors_probe_bound(uint32_t max_colors)
{
    uint32_t b = 1;
    for (uint32_t span = 1; span + 1 < max_colors; span *= 2) b++;
    return b;
}
static_assert(PLC_MAX_PROBES >= 9, "the probe list holds a search up to 256 colours");

inline PlColorsSearch pl_colors_begin(uint32_t max_colors)
{
    PlColorsSearch s;
    s.next = s.hi = max_colors;
    return s;
}

inline void pl_colors_step(PlColorsSearch &s, bool accepted)
{
    if (s.done) return;
    if (s.probes < PLC_MAX_PROBES) {
        s.probed[s.probes] = s.next;
        if (accepted) s.accepted_mask |= 1u << s.probes;
    }
    s.probes++;
    if (s.first) {
        s.first = false;
        if (!accepted) { s.chosen = s.next; s.done = true; return; }
        s.lo = 1; s.hi = s.next;
    } else if (accepted) s.hi = s.next;
    else s.lo = s.next;
    if (s.hi - s.lo > 1) s.next = (s.lo + s.hi) / 2;
    else { s.chosen = s.hi; s.reached = true; s.done = true; }
}

/* A probe that needs no device work: of an image without pixels, or at an N the image's colours fit into (colors_in: pli_colors_of's count, 257 =
 * more than 256).  Its record is all zero apart from `pixels` and it is accepted. */
inline bool pl_colors_probe_is_exact(uint64_t pixels, uint32_t colors_in, uint32_t n) { return !pixels || n >= colors_in; }

/* ... every such probe of an image taken at once.  Returns how many probes it stepped through. */
inline uint32_t pl_colors_settle(PlColorsSearch &s, uint64_t pixels, uint32_t colors_in)
{
    uint32_t stepped = 0;
    while (!s.done && pl_colors_probe_is_exact(pixels, colors_in, s.next)) { pl_colors_step(s, true); stepped++; }
    return stepped;
}

/* One round: the images still searching and the N each probes, in input order.  They run in the same launches, one job each, every job with its own
 * number of entries. */
inline std::vector<std::pair<uint32_t, uint32_t>> pl_colors_round(const std::vector<PlColorsSearch> &s)
{
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (size_t i = 0; i < s.size(); i++)
        if (!s[i].done) out.emplace_back((uint32_t)i, s[i].next);
    return out;
}

#endif

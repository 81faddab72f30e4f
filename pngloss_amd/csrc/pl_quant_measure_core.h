/*
 * pl_quant_measure_core.h -- the remap pass of the colour quantiser in a measure-only mode, as pl_deflate_measure is for the deflate: every pixel's
 * nearest entry is found as pl_quant_remap finds it (pl_quant_core.h: plq_search_quad) and the pair (pixel, entry word) goes to the distortion sums
 * (pl_distort_core.h: pld_pixel).  No pixel is stored.  Everything is an integer: the record equals pl_distort's on the remapped image bit for bit.
 * A probe of pngloss_hip_quantize_batch_target (pl_colors.h) so reads 4 bytes per pixel where a remap and a pl_distort write 4 and read 8.
 *
 * Shared by the HIP kernel (pl_quant.hip: pl_quant_measure -- one lane runs plq_measure_lane, the sums are merged through the wave, the workgroup
 * and one atomic per quantity) and by tests/c/quant_measure_host.cpp (test infrastructure), which runs the same lane loop on the CPU under the
 * sanitizers.
 */
#ifndef PL_QUANT_MEASURE_CORE_H
#define PL_QUANT_MEASURE_CORE_H

#include "pl_quant_core.h"
#include "pl_distort_core.h"

/* up to PLQ_QUAD words from p: one 16-byte load when they are whole and aligned, else word by word */
PLQ_HD void plq_load_quad(const uint32_t *p, uint32_t m, uint32_t *w)
{
    if (m == PLQ_QUAD && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const PldQuad v = *reinterpret_cast<const PldQuad *>(p);
        for (uint32_t k = 0; k < PLQ_QUAD; k++) w[k] = v.px[k];
    } else {
        for (uint32_t k = 0; k < PLQ_QUAD; k++) w[k] = k < m ? p[k] : 0u;
    }
}

/* The share of lane `lane` (of `lanes`) of workgroup `block` (of `blocks`) in an image of n pixels: the workgroup takes the chunks block,
 * block + blocks, ... of lanes * PLQ_QUAD pixels, the lane one quad of each -- the walk of pl_quant_assign and pl_quant_remap.  pal2: plq_search's
 * table of `entries` entries.  The lane's 32-bit sums are emptied into the 64-bit ones as pld_thread empties them: a workgroup may take 2^24 pixels
 * (plq_blocks), a lane so 65 536, and a step adds at most four to the PLD_FLUSH_PIXELS a lane holds. */
static_assert(PLD_FLUSH_PIXELS + PLQ_QUAD - 1 <= PLD_LANE_PIXELS_MAX, "a lane's 32-bit sums would overflow before they are flushed");
/* Visible (include/pngloss_hip_quant_space.h): the pixels are premultiplied behind the load, the entries are premultiplied words, and the sums are
 * taken on (pm(p), pal[k]) as they stand -- pm(plq_straight(pal[k])) == pal[k], so this is the visible-mode record of (input, remapped image) without
 * the straight word ever being made.  s.visible counts the pixels whose alpha or whose entry's alpha is non-zero. */
template <bool Visible = false>
PLQ_HD PldSum plq_measure_lane(const uint32_t *pal2, uint32_t entries, const uint32_t *img, size_t n, size_t block, size_t blocks, uint32_t lane, uint32_t lanes)
{
    PldSum s = {};
    PldLane l = {};
    uint32_t held = 0;
    const size_t chunk = (size_t)lanes * PLQ_QUAD;
    for (size_t c = block; c * chunk < n; c += blocks) {
        const size_t base = c * chunk + (size_t)lane * PLQ_QUAD;
        if (base >= n) continue;
        const uint32_t m = n - base < PLQ_QUAD ? (uint32_t)(n - base) : PLQ_QUAD;
        uint32_t w[PLQ_QUAD], best[PLQ_QUAD];
        plq_load_quad(img + base, m, w);
        plq_space_quad<Visible>(w, m);
        plq_search_quad(pal2, entries, w, m, best);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < PLQ_QUAD; k++)
            if (k < m) {
                pld_pixel(l, w[k], pal2[2 * best[k]]);
                if (Visible) l.visible += ((w[k] | pal2[2 * best[k]]) >> 24) ? 1u : 0u;
            }
        held += m;
        if (held >= PLD_FLUSH_PIXELS) { pld_flush(s, l); held = 0; }
    }
    pld_flush(s, l);
    return s;
}

#endif

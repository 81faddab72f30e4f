/*
 * pl_dither_core.h -- the logic of the quantiser's error diffusion (include/pngloss_hip_dither.h): the step of one pixel, and the schedule by which
 * one workgroup walks an image whose every pixel depends on its left and its upper-right neighbour.  No reference equivalent.
 *
 * The rule (all integers; restated as a plain raster loop in tests/util_dither.py).  Pixels in raster order, y then x ascending.  e_c(y, x) is the
 * signed error of channel c at a visited pixel, 0 outside the image.
 *   S_c = 7 e_c(y, x-1) + 1 e_c(y-1, x-1) + 5 e_c(y-1, x) + 3 e_c(y-1, x+1)
 *   a_c = p_c(y, x) + floor((S_c + 8) / 16),  v_c = min(255, max(0, a_c)),  v the RGBA8 word of the four v_c
 *   k   = the entry nearest to v (plq_search<1>: smallest squared distance over four channels, lowest index among equals)
 *   the output pixel is pal[k], and e_c(y, x) = v_c - pal[k]_c
 *
 * The schedule.  Pixel (y, x) needs (y, x-1) and (y-1, x+1): row y may be at column x once row y-1 has finished column x+1, a skew of PLF_SKEW = 2
 * columns a row.  One workgroup takes one image.  A lane has a row; a wave holds PLF_LANES consecutive rows and walks them in lock-step: at the
 * wave's local step t lane r is at column t - 2r (plf_column), so a wave needs plf_wave_epochs(W) * PLF_K local steps for a width W.  A lane keeps
 * its newest error (`last`: 0 while its column is outside the image) and the three errors above its pixel in registers; every step it takes the
 * newest error of the lane above it -- column x+1 of the row above -- with one cross-lane move.  The PLF_WAVES waves of the workgroup hold a band
 * of PLF_BAND rows.  Lane 63 of wave k-1 leaves its errors in wave k's ring in LDS (plf_ring_index), where lane 0 of wave k finds them.  No lane
 * waits on memory: the waves advance in epochs of PLF_K local steps with one barrier per epoch, and wave k runs PLF_LAG epochs behind wave k-1
 * (plf_local_epoch) -- the wave above reaches column x+1 at its local step x + 127, and in the epoch in which wave k is at local steps
 * j*K .. j*K + K-1 the wave above has finished its local step (j + PLF_LAG) * K - 1 >= j*K + K-1 + 127.  Every wave executes every barrier of the
 * band, plf_band_epochs of them, idle or not.  Bands follow one another in the workgroup; the last row of a band leaves its errors in the image's
 * error line in the workspace (W entries), which lane 0 of wave 0 of the next band reads.
 *
 * Shared by the HIP kernel (pl_dither.hip) and by tests/c/dither_host.cpp (test infrastructure), which runs the kernel's own order on the CPU -- band
 * by band, epoch by epoch, wave by wave, the lanes as a loop -- under the sanitizers.
 */
#ifndef PL_DITHER_CORE_H
#define PL_DITHER_CORE_H

#include "pl_quant_core.h"

constexpr uint32_t PLF_LANES = 64;                       /* rows of a wave */
#ifdef PLF_MEASURE_WAVES                                 /* (a variant library for tools/dither_profile.py: 4 .. 16, DESIGN.md 9.1c has the figures) */
constexpr uint32_t PLF_WAVES = PLF_MEASURE_WAVES;
#else
constexpr uint32_t PLF_WAVES = 16;                       /* waves of the workgroup */
#endif
constexpr uint32_t PLF_BAND = PLF_LANES * PLF_WAVES;     /* rows of a band */
constexpr uint32_t PLF_K = 64;                           /* local steps of an epoch */
constexpr uint32_t PLF_SKEW = 2;                         /* columns a row runs behind the row above it */
constexpr uint32_t PLF_REACH = PLF_SKEW * (PLF_LANES - 1) + 1;   /* lane 63 finishes column x+1 at its wave's local step x + PLF_REACH */
constexpr uint32_t PLF_LAG = (PLF_REACH + PLF_K - 1 + PLF_K) / PLF_K;   /* epochs wave k runs behind wave k-1 */
constexpr uint32_t PLF_RING = 256;                       /* entries of a wave's ring: a power of two */
constexpr uint32_t PLF_RING_ENTRIES = PLF_WAVES * PLF_RING;      /* (ring 0 has no writer: wave 0 reads the error line) */
static_assert(PLF_WAVES >= 4 && PLF_WAVES <= 16 && PLF_LANES == 64, "a workgroup of 256 .. 1024 lanes, a wave of 64");
static_assert(PLF_REACH == 127 && PLF_K == 64 && PLF_LAG == 3, "with K = 64 the lag is three epochs: they cover 127 + 63 local steps");
static_assert(PLF_LAG * PLF_K >= PLF_REACH + PLF_K, "when wave k starts an epoch the wave above has finished what the epoch's last step needs");
/* In one epoch the reader is at columns c+1 for its K local steps and the writer PLF_LAG epochs on, PLF_SKEW * 63 columns back: the columns that are
 * live at the same time span PLF_LAG * K + K - PLF_SKEW * 63 of them, and a slot is written again only a whole epoch after its reader has passed */
static_assert((PLF_RING & (PLF_RING - 1)) == 0 && PLF_RING >= PLF_LAG * PLF_K + 2 * PLF_K - PLF_SKEW * (PLF_LANES - 1), "no ring slot is written before its reader has passed it");

/* the bounds of the rule */
constexpr int32_t PLF_MAX_E = 255, PLF_MAX_S = (7 + 1 + 5 + 3) * PLF_MAX_E;
static_assert(PLF_MAX_E <= INT16_MAX, "|e_c| <= 255: an error fits 16 bits");
static_assert(PLF_MAX_S == 4080, "|S_c| <= 4080");
static_assert(0 + (-PLF_MAX_S + 8 - 15) / 16 == -255 && 255 + (PLF_MAX_S + 8) / 16 == 510, "-255 <= a_c <= 510 (the first quotient rounded down by hand)");
constexpr int32_t PLF_FLOOR_BIAS = 4096;                 /* a multiple of 16 above PLF_MAX_S - 8: the shift below never sees a negative number */
static_assert(PLF_FLOOR_BIAS % 16 == 0 && PLF_FLOOR_BIAS >= PLF_MAX_S - 8, "S + 8 + bias >= 0");

/* the four errors of a pixel, 16 bits each: channel 0 in the low half of lo, 1 in its high half, 2 and 3 in hi.  (the error line and the rings hold these) */
struct PlfErr { uint32_t lo, hi; };
constexpr size_t PLF_ERR_BYTES = 8;
static_assert(sizeof(PlfErr) == PLF_ERR_BYTES, "W x 4 x int16");

PLQ_HD int32_t plf_err_channel(PlfErr e, uint32_t c)
{
    const uint32_t half = ((c < 2 ? e.lo : e.hi) >> (16 * (c & 1u))) & 0xFFFFu;
    return (int32_t)half - (int32_t)((half & 0x8000u) << 1);
}
PLQ_HD PlfErr plf_err_pack(const int32_t e[4])
{
    PlfErr r;
    r.lo = ((uint32_t)e[0] & 0xFFFFu) | ((uint32_t)e[1] << 16);
    r.hi = ((uint32_t)e[2] & 0xFFFFu) | ((uint32_t)e[3] << 16);
    return r;
}

/* floor((S + 8) / 16) for |S| <= PLF_MAX_S */
PLQ_HD int32_t plf_round16(int32_t s) { return (int32_t)((uint32_t)(s + 8 + PLF_FLOOR_BIAS) >> 4) - PLF_FLOOR_BIAS / 16; }

/* ---- the step of one pixel ---- */

/* p: the pixel; left, ul, up, ur: the errors at (y, x-1), (y-1, x-1), (y-1, x), (y-1, x+1).  Returns the word of the nearest entry, *err the new
 * error.  pal2 as plq_search takes it.  a: when not NULL, the four a_c (the CPU harness reports them).
 * Visible (include/pngloss_hip_quant_space.h): the rule on the premultiplied pixel pm(p) over premultiplied entries; a pixel with alpha 0 takes no
 * error in (S_c counts as 0, so v = 0) and passes its own on; the word returned is straight[best], the plq_straight of the nearest entry, and the
 * error stays in premultiplied units.  The bounds of the rule hold as they are: pm(p)'s channels are 0 .. 255. */
template <bool Visible = false>
PLQ_HD uint32_t plf_pixel(const uint32_t *pal2, uint32_t entries, uint32_t p, PlfErr left, PlfErr ul, PlfErr up, PlfErr ur, PlfErr *err, int32_t *a,
                          const uint32_t *straight = nullptr)
{
    int32_t v[4];
    uint32_t word = 0;
    if (Visible) p = pld_pm(p);
    const bool takes = !Visible || (p >> 24) != 0;
    for (uint32_t c = 0; c < 4; c++) {
        const int32_t s = takes ? 7 * plf_err_channel(left, c) + plf_err_channel(ul, c) + 5 * plf_err_channel(up, c) + 3 * plf_err_channel(ur, c) : 0;
        const int32_t ac = (int32_t)plq_channel(p, c) + plf_round16(s);
        if (a) a[c] = ac;
        v[c] = ac < 0 ? 0 : ac > 255 ? 255 : ac;
        word |= (uint32_t)v[c] << (8 * c);
    }
    uint32_t best = 0;
    plq_search<1>(pal2, entries, &word, &best);
    const uint32_t out = pal2[2 * best];
    for (uint32_t c = 0; c < 4; c++) v[c] -= (int32_t)plq_channel(out, c);
    *err = plf_err_pack(v);
    return Visible ? straight[best] : out;
}

/* what a lane keeps between its steps */
struct PlfLane { PlfErr last, ul, up, ur; };

/* the lane moves one column on: the window above it shifts, `fetch` -- the newest error of the row above, column x+1 -- enters it */
PLQ_HD void plf_lane_shift(PlfLane &s, PlfErr fetch) { s.ul = s.up; s.up = s.ur; s.ur = fetch; }

/* ---- the schedule ---- */

/* the column of lane r at its wave's local step t (outside 0 .. W-1: the lane idles) */
PLQ_HD int64_t plf_column(uint64_t t, uint32_t lane) { return (int64_t)t - (int64_t)(PLF_SKEW * lane); }
/* local epochs a wave needs for a row of W pixels: lane 63 reaches column W-1 at local step W-1 + 126 */
PLQ_HD uint64_t plf_wave_epochs(uint32_t width) { return ((uint64_t)width + PLF_SKEW * (PLF_LANES - 1) + PLF_K - 1) / PLF_K; }
/* bands of an image, rows of band b, waves of a band that have rows */
PLQ_HD uint32_t plf_bands(uint32_t height) { return (uint32_t)(((uint64_t)height + PLF_BAND - 1) / PLF_BAND); }
PLQ_HD uint32_t plf_band_rows(uint32_t height, uint32_t band)
{
    const uint64_t first = (uint64_t)band * PLF_BAND;
    return height - first < PLF_BAND ? (uint32_t)(height - first) : PLF_BAND;
}
PLQ_HD uint32_t plf_band_waves(uint32_t rows) { return (rows + PLF_LANES - 1) / PLF_LANES; }
/* epochs -- barriers -- of a band whose first `waves` waves have rows: the last of them starts PLF_LAG * (waves - 1) epochs late */
PLQ_HD uint64_t plf_band_epochs(uint32_t width, uint32_t waves) { return waves ? plf_wave_epochs(width) + (uint64_t)PLF_LAG * (waves - 1) : 0; }
/* the local epoch of wave k in the band's epoch g: the wave works when it is in 0 .. plf_wave_epochs - 1 */
PLQ_HD int64_t plf_local_epoch(uint64_t g, uint32_t wave) { return (int64_t)g - (int64_t)(PLF_LAG * wave); }
/* barriers every wave of the workgroup executes for an image */
PLQ_HD uint64_t plf_barriers(uint32_t width, uint32_t height)
{
    if (!width || !height) return 0;
    const uint32_t bands = plf_bands(height);
    return (uint64_t)(bands - 1) * plf_band_epochs(width, PLF_WAVES) + plf_band_epochs(width, plf_band_waves(plf_band_rows(height, bands - 1)));
}
/* where the error of column x of the last row of wave k-1 lies in the rings: reader_wave = k */
PLQ_HD uint32_t plf_ring_index(uint32_t reader_wave, uint64_t column) { return reader_wave * PLF_RING + (uint32_t)(column & (PLF_RING - 1)); }

#endif

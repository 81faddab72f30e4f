/*
 * pl_quant_core.h -- the logic of the colour quantiser (include/pngloss_hip_quant.h): make an RGBA8 image have at most N colours, so that the indexed
 * write side (pl_index_core.h) finds a palette.  No reference equivalent (the reference tool never reduces colours).
 *
 * Definitions (all integers, all exact; restated with numpy and Python integers in tests/util_quant.py).  A pixel is its RGBA8 word, channels R, G, B, A
 * in that order (R in the low byte).  Parameters: max_colors N in 2..256, rounds R in 0..64.
 *   exact        an image with at most N distinct words comes back unchanged, exact = 1, its palette its colours ascending by word (the indexed
 *                side's order).  pl_index_count decides it (its counter is exact up to 256).  An image without pixels is exact with 0 entries.
 *   histogram    bin(p) = (R>>4) | (G>>4)<<4 | (B>>4)<<8 | (A>>4)<<12: 65 536 bins of 32-bit counts; a bin's coordinate on channel c is that 4-bit field
 *   median cut   on the host, over the non-empty bins.  A box is a list of bins, its range on a channel the max minus the min coordinate.  Start: one box
 *                of every non-empty bin in ascending bin order.  While there are fewer than N boxes and some box has a non-zero range: take the box with
 *                the largest pixel count among those with a non-zero range (tie: the first in the list); the channel with the largest range (tie: the
 *                lowest); lo, hi = its smallest and largest coordinate in the box; the cut t = the smallest value in lo .. hi-1 for which twice the
 *                pixels with coordinate <= t is at least the box's pixel count, hi-1 if there is none; the box is replaced in place by (coordinate <= t)
 *                and then (coordinate > t), each in ascending bin order.  A box's colour is per channel (2*S + P) / (2*P), floor, with S the sum over its
 *                bins of count * (16 * coordinate + 8) and P its pixel count.  The result: an initial palette of 1..N entries, in list order.
 *   refinement   R rounds: every pixel goes to the entry with the smallest squared distance over the four channels (tie: the lowest index); per entry the
 *                pixel count and the four 64-bit channel sums; an entry with a count becomes (2*sum + count) / (2*count) per channel, floor, one
 *                without stays.  Integer sums do not depend on the order: any grid gives the same palette.
 *   remap        every pixel becomes the word of its nearest entry of the final palette.  Entries may be duplicates or unused: the REPORTED palette is
 *                the distinct words of the remapped image, ascending -- what the indexed side will find.
 *
 * The search.  |p - c|^2 = |p|^2 + |c|^2 - 2 p.c, and |p|^2 is the pixel's own: the order of the entries is that of |c|^2 - 2 p.c.  An entry's key for a
 * pixel is ((2 p.c - |c|^2 + PLQ_BIAS) << 8) | (255 - index): the LARGEST key is the nearest entry, and among equals the lowest index.  An entry keeps
 * its word and its base = ((PLQ_BIAS - |c|^2) << 8) | (255 - index); key = (p.c << 9) + base -- on the device one v_dot4_u32_u8, one v_lshl_add_u32 and
 * one v_max_u32 per pixel and entry.
 *
 * The space (include/pngloss_hip_quant_space.h).  With Visible every step above runs on the alpha-premultiplied words pm(p) (pl_distort_core.h: pld_pm)
 * instead of p: a pixel is converted once, right behind its load (plq_space_quad), and everything behind that -- bins, keys, sums, the merging of equal
 * neighbours -- sees premultiplied words.  The palette holds premultiplied words; what the remap stores is plq_straight of the entry.  Without Visible
 * nothing is converted and the code is what it was.
 *
 * Shared by the HIP kernels (pl_quant.hip) and by tests/c/quant_host.cpp and tests/c/quant_space_host.cpp (test infrastructure), which run the same
 * bodies on the CPU under the sanitizers, with one thread and with a team of threads that accumulate concurrently.
 */
#ifndef PL_QUANT_CORE_H
#define PL_QUANT_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "pl_distort_core.h"

#if defined(__HIPCC__)
#define PLQ_HD __host__ __device__ __forceinline__
#else
#define PLQ_HD inline
#endif

constexpr uint32_t PLQ_MIN_COLORS = 2, PLQ_MAX_COLORS = 256, PLQ_MAX_ROUNDS = 64;
constexpr uint32_t PLQ_BINS = 65536;
constexpr uint32_t PLQ_QUAD = 4;                    /* pixels per thread and step: one 16-byte load */
constexpr uint32_t PLQ_CELLS = 5;                   /* per entry: the pixel count and the four channel sums */
constexpr uint32_t PLQ_BIAS = 1u << 19;             /* above 4 * 255^2 = 260 100, the largest |c|^2 and the largest p.c */
static_assert(4u * 255u * 255u < PLQ_BIAS && ((uint64_t)(2u * 4u * 255u * 255u + PLQ_BIAS) << 8) < ((uint64_t)1 << 32), "a key fits 32 bits and never goes below zero");

/* A workgroup accumulates in 32-bit cells: the largest sum of one channel over the pixels it takes has to fit */
constexpr uint64_t PLQ_WG_PIXELS = (uint64_t)1 << 24;
static_assert(255ull * PLQ_WG_PIXELS < ((uint64_t)1 << 32), "a workgroup's 32-bit cells hold the channel sums of all its pixels");
constexpr uint32_t PLQ_MAX_BLOCKS = 1024;           /* workgroups per image of the assign pass at most */
/* A larger image is refused (PNGLOSS_INVALID_ARGUMENT).  A histogram bin is a 32-bit count and one bin may take every pixel of an image: the pixel
 * count has to fit it.  (The grid alone would allow PLQ_WG_PIXELS * PLQ_MAX_BLOCKS = 2^34.) */
constexpr uint64_t PLQ_MAX_PIXELS = ((uint64_t)1 << 32) - 1;
static_assert(PLQ_MAX_PIXELS <= UINT32_MAX, "a histogram bin's 32-bit count holds every pixel of an image");
static_assert(PLQ_MAX_PIXELS <= PLQ_WG_PIXELS * PLQ_MAX_BLOCKS, "the largest grid takes the largest image with no workgroup past PLQ_WG_PIXELS");
PLQ_HD bool plq_pixels_ok(uint64_t pixels) { return pixels <= PLQ_MAX_PIXELS; }

#if defined(__HIP_DEVICE_COMPILE__)
#define PLQ_ADD32(p, v) atomicAdd((p), (v))
#define PLQ_ADD64(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#define PLQ_DOT4(a, b) __builtin_amdgcn_udot4((a), (b), 0u, false)
#else
#define PLQ_ADD32(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define PLQ_ADD64(p, v) ((void)__atomic_fetch_add((p), (v), __ATOMIC_RELAXED))
#define PLQ_DOT4(a, b) plq_dot4_plain((a), (b))
#endif

PLQ_HD uint32_t plq_channel(uint32_t word, uint32_t c) { return (word >> (8 * c)) & 255u; }
PLQ_HD uint32_t plq_dot4_plain(uint32_t a, uint32_t b)
{
    return plq_channel(a, 0) * plq_channel(b, 0) + plq_channel(a, 1) * plq_channel(b, 1) + plq_channel(a, 2) * plq_channel(b, 2) + plq_channel(a, 3) * plq_channel(b, 3);
}

/* ---- the space ---- */

/* the m <= PLQ_QUAD pixels a lane has just loaded, as the words the search runs on */
template <bool Visible>
PLQ_HD void plq_space_quad(uint32_t *w, uint32_t m)
{
    if (Visible)
        for (uint32_t k = 0; k < PLQ_QUAD; k++)
            if (k < m) w[k] = pld_pm(w[k]);
}

/* the straight word of a premultiplied palette entry: alpha 0 is the word 0, else each of R, G, B is (c' * 255 + a / 2) / a, at most 255.
 * pm(plq_straight(e)) == e whenever r', g', b' <= a, which holds for every entry made of premultiplied pixels (tests/test_quant_space_host.py) */
PLQ_HD uint32_t plq_straight(uint32_t entry)
{
    const uint32_t a = entry >> 24;
    if (!a) return 0u;
    uint32_t word = entry & 0xFF000000u;
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t v = (plq_channel(entry, c) * 255u + a / 2u) / a;
        word |= (v > 255u ? 255u : v) << (8 * c);
    }
    return word;
}

/* ---- the histogram ---- */

PLQ_HD uint32_t plq_bin(uint32_t word)
{
    return ((word >> 4) & 15u) | (((word >> 12) & 15u) << 4) | (((word >> 20) & 15u) << 8) | (((word >> 28) & 15u) << 12);
}
PLQ_HD uint32_t plq_coord(uint32_t bin, uint32_t c) { return (bin >> (4 * c)) & 15u; }

/* m <= PLQ_QUAD consecutive pixels into the table: a run of pixels of one bin costs one atomic.  Visible: the bins of the premultiplied words.
 * There every pixel with an alpha below 16 lands in bin 0, whatever its colour -- the whole transparent surround of a sprite, millions of additions
 * to one address.  With held0 they go to the caller's own count instead, which it adds to hist[0] once (pl_quant_hist_visible: once per wave). */
template <bool Visible = false>
PLQ_HD void plq_hist_quad(uint32_t *hist, const uint32_t *w, uint32_t m, uint32_t *held0 = nullptr)
{
    uint32_t bin = 0, run = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t b = plq_bin(Visible ? pld_pm(w[k]) : w[k]);
        if (run && b != bin) {
            if (Visible && held0 && !bin) *held0 += run;
            else PLQ_ADD32(hist + bin, run);
            run = 0;
        }
        bin = b; run++;
    }
    if (run) {
        if (Visible && held0 && !bin) *held0 += run;
        else PLQ_ADD32(hist + bin, run);
    }
}

/* ---- the grid of the assign pass: how many workgroups an image gets, and how many pixels the busiest of them takes ---- */

/* chunk: the pixels a workgroup takes per step (threads * PLQ_QUAD); want: the workgroups the launch would like.  Workgroup b takes the chunks
 * b, b + blocks, b + 2 * blocks, ... */
inline uint32_t plq_blocks(uint64_t pixels, uint64_t chunk, uint32_t want)
{
    const uint64_t chunks = (pixels + chunk - 1) / chunk;
    uint64_t need = (pixels + PLQ_WG_PIXELS - 1) / PLQ_WG_PIXELS * 2;      /* (twice: a workgroup takes whole chunks, its share is rounded up) */
    if (need > PLQ_MAX_BLOCKS) need = PLQ_MAX_BLOCKS;
    uint64_t blocks = want > need ? want : need;
    if (blocks > chunks) blocks = chunks;
    if (blocks > PLQ_MAX_BLOCKS) blocks = PLQ_MAX_BLOCKS;
    return blocks ? (uint32_t)blocks : 1u;
}
inline uint64_t plq_wg_pixels(uint64_t pixels, uint64_t chunk, uint32_t blocks)
{
    const uint64_t chunks = (pixels + chunk - 1) / chunk;
    return (chunks + blocks - 1) / blocks * chunk;
}

/* ---- the search ---- */

/* what an entry keeps beside its word */
PLQ_HD uint32_t plq_base(uint32_t word, uint32_t index) { return ((PLQ_BIAS - plq_dot4_plain(word, word)) << 8) | (255u - index); }
PLQ_HD uint32_t plq_key(uint32_t dot, uint32_t base) { return (dot << 9) + base; }
PLQ_HD uint32_t plq_index_of_key(uint32_t key) { return 255u - (key & 255u); }

/* the nearest of `entries` entries for M pixels at once.  pal2: entry e's word at [2 * e], its base at [2 * e + 1] -- on the device in LDS, one
 * 8-byte read per entry, and every lane reads the same entry: a broadcast */
template <uint32_t M>
PLQ_HD void plq_search(const uint32_t *pal2, uint32_t entries, const uint32_t *w, uint32_t *best)
{
    uint32_t key[M];
    for (uint32_t i = 0; i < M; i++) key[i] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (uint32_t e = 0; e < entries; e++) {
        const uint32_t c = pal2[2 * e], b = pal2[2 * e + 1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < M; i++) {
            const uint32_t k = plq_key(PLQ_DOT4(w[i], c), b);
            key[i] = k > key[i] ? k : key[i];
        }
    }
    for (uint32_t i = 0; i < M; i++) best[i] = plq_index_of_key(key[i]);
}

/* m <= PLQ_QUAD consecutive pixels: best[k] = the entry of pixel k.  A pixel equal to the one before it reuses its answer: a quad of one colour
 * is searched once */
PLQ_HD void plq_search_quad(const uint32_t *pal2, uint32_t entries, const uint32_t *w, uint32_t m, uint32_t *best)
{
    bool flat = true;
    for (uint32_t k = 1; k < m; k++) flat = flat && w[k] == w[0];
    if (flat) {
        uint32_t one = 0;
        plq_search<1>(pal2, entries, w, &one);
        for (uint32_t k = 0; k < PLQ_QUAD; k++) best[k] = one;
        return;
    }
    uint32_t q[PLQ_QUAD];
    for (uint32_t k = 0; k < PLQ_QUAD; k++) q[k] = k < m ? w[k] : w[0];
    plq_search<PLQ_QUAD>(pal2, entries, q, best);
}

/* ... added to a workgroup's cells (cells[entry * PLQ_CELLS + 0] the count, + 1 + c the sum of channel c): a run of equal pixels costs one
 * addition per cell */
PLQ_HD void plq_accumulate_quad(uint32_t *cells, const uint32_t *w, const uint32_t *best, uint32_t m)
{
    for (uint32_t k = 0; k < m;) {
        uint32_t run = 1;
        while (k + run < m && w[k + run] == w[k]) run++;
        uint32_t *cell = cells + best[k] * PLQ_CELLS;
        PLQ_ADD32(cell, run);
        for (uint32_t c = 0; c < 4; c++) {
            const uint32_t v = plq_channel(w[k], c) * run;
            if (v) PLQ_ADD32(cell + 1 + c, v);
        }
        k += run;
    }
}

/* a workgroup's cell into the image's 64-bit accumulator: one atomic, none for a cell that is zero */
PLQ_HD void plq_flush_cell(uint64_t *acc, const uint32_t *cells, uint32_t i)
{
    if (cells[i]) PLQ_ADD64(acc + i, (uint64_t)cells[i]);
}

/* ---- the update: entry k from its accumulator, which is zeroed for the next round ---- */

PLQ_HD uint32_t plq_mean(uint64_t sum, uint64_t count) { return (uint32_t)((2 * sum + count) / (2 * count)); }

PLQ_HD void plq_update_entry(uint32_t *pal, uint64_t *acc, uint32_t k)
{
    uint64_t *a = acc + (size_t)k * PLQ_CELLS;
    if (a[0]) pal[k] = plq_mean(a[1], a[0]) | plq_mean(a[2], a[0]) << 8 | plq_mean(a[3], a[0]) << 16 | plq_mean(a[4], a[0]) << 24;
    for (uint32_t c = 0; c < PLQ_CELLS; c++) a[c] = 0;
}

/* ---- the median cut (host) ---- */

#include <vector>

struct PlqBox {
    std::vector<uint32_t> bins;     /* ascending */
    uint64_t pixels = 0;
    uint32_t lo[4] = {}, hi[4] = {};
};

inline void plq_box_measure(PlqBox &b, const uint32_t *hist)
{
    b.pixels = 0;
    for (uint32_t c = 0; c < 4; c++) { b.lo[c] = 15; b.hi[c] = 0; }
    for (uint32_t bin : b.bins) {
        b.pixels += hist[bin];
        for (uint32_t c = 0; c < 4; c++) {
            const uint32_t v = plq_coord(bin, c);
            if (v < b.lo[c]) b.lo[c] = v;
            if (v > b.hi[c]) b.hi[c] = v;
        }
    }
}
inline uint32_t plq_box_range(const PlqBox &b)
{
    uint32_t r = 0;
    for (uint32_t c = 0; c < 4; c++) if (b.hi[c] - b.lo[c] > r) r = b.hi[c] - b.lo[c];
    return r;
}
inline uint32_t plq_box_colour(const PlqBox &b, const uint32_t *hist)
{
    uint64_t s[4] = {};
    for (uint32_t bin : b.bins)
        for (uint32_t c = 0; c < 4; c++) s[c] += (uint64_t)hist[bin] * (16u * plq_coord(bin, c) + 8u);
    return plq_mean(s[0], b.pixels) | plq_mean(s[1], b.pixels) << 8 | plq_mean(s[2], b.pixels) << 16 | plq_mean(s[3], b.pixels) << 24;
}

/* hist: PLQ_BINS counts, at least one of them non-zero.  Returns the initial palette: 1 .. max_colors words, in list order */
inline std::vector<uint32_t> plq_median_cut(const uint32_t *hist, uint32_t max_colors)
{
    std::vector<PlqBox> boxes(1);
    for (uint32_t bin = 0; bin < PLQ_BINS; bin++) if (hist[bin]) boxes[0].bins.push_back(bin);
    if (boxes[0].bins.empty()) return {};
    plq_box_measure(boxes[0], hist);
    while (boxes.size() < max_colors) {
        size_t pick = boxes.size();
        for (size_t i = 0; i < boxes.size(); i++)
            if (plq_box_range(boxes[i]) && (pick == boxes.size() || boxes[i].pixels > boxes[pick].pixels)) pick = i;
        if (pick == boxes.size()) break;
        const PlqBox &box = boxes[pick];
        uint32_t ch = 0;
        for (uint32_t c = 1; c < 4; c++) if (box.hi[c] - box.lo[c] > box.hi[ch] - box.lo[ch]) ch = c;
        uint64_t at[16] = {};
        for (uint32_t bin : box.bins) at[plq_coord(bin, ch)] += hist[bin];
        uint32_t t = box.hi[ch] - 1;
        uint64_t cum = 0;
        for (uint32_t v = box.lo[ch]; v < box.hi[ch]; v++) {
            cum += at[v];
            if (2 * cum >= box.pixels) { t = v; break; }
        }
        PlqBox low, high;
        for (uint32_t bin : box.bins) (plq_coord(bin, ch) <= t ? low : high).bins.push_back(bin);
        plq_box_measure(low, hist);
        plq_box_measure(high, hist);
        boxes[pick] = low;
        boxes.insert(boxes.begin() + (long)pick + 1, high);
    }
    std::vector<uint32_t> pal;
    for (const PlqBox &b : boxes) pal.push_back(plq_box_colour(b, hist));
    return pal;
}

#endif

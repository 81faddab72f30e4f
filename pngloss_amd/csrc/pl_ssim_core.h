/*
 * pl_ssim_core.h -- the arithmetic of the structural similarity measurement (SSIM): how much of the original's local mean and structure the optimised
 * RGBA8 image keeps.  No reference equivalent (the reference tool reports file sizes only).  include/pngloss_hip.h states the definition for
 * callers; in short, per image, over its pixel pairs (a = original, b = optimised; channel c in byte c of the pixel word):
 *     windows      8x8 pixels at a stride of 4 in both directions: origins (4i, 4j), i < nx, j < ny  (the layout x264 and libvpx use)
 *     per window and channel, from the five sums over its 64 pixels, q = sign(num) * floor(|num| * 65536 / den)   (pls_q16)
 *     sum_q16[c]   sum of q over the windows; min_q16[c] the smallest q (65536 without windows)
 * Everything is an integer, so the record does not depend on the order the windows are summed in: the kernel's lanes and a loop on the CPU give
 * the same 64 bytes.
 *
 * A window is 2x2 CELLS of 4x4 pixels, and a cell belongs to up to four windows, so the sums are taken per cell and added per window.  The image
 * is cut into tiles of PLS_TILE_WX x PLS_TILE_WY window origins; a window belongs to the tile that holds its origin.  A tile's cells -- one more
 * column and row of them than it has windows: the halo its last windows reach into -- are summed into a table (LDS on the device), then every
 * window of the tile is formed from the table.
 *
 * Shared by the HIP kernel (pl_ssim.hip: a workgroup per tile, thread t runs pls_thread_cells and pls_thread_windows, the partial records are
 * merged through the wave, the workgroup and one atomic per quantity) and by tests/c/ssim_host.cpp and tests/c/visible_host.cpp (test
 * infrastructure), which run the same two thread loops on the CPU under the sanitizers.  In visible mode (the <true> instantiations; below) the
 * sums are those of alpha-premultiplied pixels and only windows that hold a visible pixel count.
 */
#ifndef PL_SSIM_CORE_H
#define PL_SSIM_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLS_HD __host__ __device__ __forceinline__
#else
#define PLS_HD inline
#endif

/* the record of one image as the kernel writes it: the layout of pngloss_hip_ssim (include/pngloss_hip.h; pl_host_ctx.h asserts it) */
struct PlSsimRecord {
    uint64_t windows;
    int64_t sum_q16[4];
    int32_t min_q16[4];
    uint64_t reserved;
};
static_assert(sizeof(PlSsimRecord) == 64, "PlSsimRecord: six 64-bit words and four 32-bit ones, no padding");

constexpr uint32_t PLS_WINDOW = 8, PLS_STRIDE = 4, PLS_CELL = 4;       /* pixels: a window is 2x2 cells, the stride is one cell */
constexpr int32_t PLS_ONE = 65536;                                     /* q of two equal windows */
/* 64^2 * (0.01 * 255)^2 and 64^2 * (0.03 * 255)^2, rounded */
constexpr uint64_t PLS_K1 = 26634, PLS_K2 = 239708;

/* the bounds of the window arithmetic (pls_q16), from 64 pixels of at most 255 */
constexpr uint64_t PLS_S_MAX = 64 * 255;                               /* sa, sb: 16 320 */
constexpr uint64_t PLS_B1_MAX = 2 * PLS_S_MAX * PLS_S_MAX + PLS_K1;    /* A1 <= B1 */
/* B2 is 64^2 times the sum of the two variances, + K2: largest for half the pixels 0 and half 255 in both windows.  |A2| <= B2, since A2 is 64^2
 * times twice the covariance, + K2 (Cauchy-Schwarz). */
constexpr uint64_t PLS_B2_MAX = 2 * (64 * 32 * 255 * 255 - (32 * 255) * (32 * 255)) + PLS_K2;
static_assert(PLS_S_MAX == 16320, "sa, sb <= 16320");
static_assert(PLS_B1_MAX < (1ull << 29), "A1, B1 < 2^29");
static_assert(PLS_B2_MAX * 1000 < (1ull << 27) * 1071, "B2 < 2^27.1 (2^0.1 = 1.0717...)");
static_assert(PLS_B1_MAX * PLS_B2_MAX < (1ull << 57), "|num| <= den < 2^57");

/* the sums of a 4x4 cell and one channel: 16 pixels, so sa and sb fit 12 bits (packed: sa in the low half of `s`, sb in the high half) and
 * saa, sbb, sab fit 20 bits.  Four 32-bit words: one 16-byte LDS access. */
struct alignas(16) PlsCell { uint32_t s, aa, bb, ab; };
static_assert(16 * 255 < (1 << 12) && 16 * 255 * 255 < (1 << 20), "cell sums: 12 and 20 bits");

/* four pixels behind one 16-byte load */
struct alignas(16) PlsQuad { uint32_t px[4]; };

/* ---- geometry: windows, cells and tiles of a width x height image ---- */
constexpr uint32_t PLS_TILE_WX = 32, PLS_TILE_WY = 8;                  /* window origins per tile: 128 x 32 pixels */
constexpr uint32_t PLS_TILE_CX = PLS_TILE_WX + 1, PLS_TILE_CY = PLS_TILE_WY + 1;       /* cells per tile, with the halo */
constexpr uint32_t PLS_TILE_CELLS = PLS_TILE_CX * PLS_TILE_CY;         /* 297: the table holds 4 channels of each, 19 008 bytes */
constexpr uint32_t PLS_TILE_ITEMS = PLS_TILE_WX * PLS_TILE_WY * 4;     /* (window, channel) pairs per tile: 1024 */

struct PlsGeom {
    uint32_t nx, ny;            /* windows per row and column of the image */
    uint32_t tiles_x, tiles_y;
    uint64_t windows, tiles;
};

PLS_HD PlsGeom pls_geom(uint32_t width, uint32_t height)
{
    PlsGeom g;
    g.nx = width >= PLS_WINDOW ? (width - PLS_WINDOW) / PLS_STRIDE + 1 : 0;
    g.ny = height >= PLS_WINDOW ? (height - PLS_WINDOW) / PLS_STRIDE + 1 : 0;
    if (!g.nx || !g.ny) g.nx = g.ny = 0;
    g.tiles_x = (g.nx + PLS_TILE_WX - 1) / PLS_TILE_WX;
    g.tiles_y = (g.ny + PLS_TILE_WY - 1) / PLS_TILE_WY;
    g.windows = (uint64_t)g.nx * g.ny;
    g.tiles = (uint64_t)g.tiles_x * g.tiles_y;
    return g;
}

/* ---- the launch shape of pl_ssim (pl_ssim.hip), stated here so that a CPU test can pin it: a launch takes at most PLS_MAX_IMAGES images (gridDim.y; a
 * larger batch is launched in slices), and an image gets a workgroup per tile of the batch's largest image, but only as many as fill 256 CUs several
 * times over across the batch (pl_distort_core.h:pld_grid_blocks has the same cap): min(max_tiles, max(8, ceil(2048 / n))), at least 1.  Workgroup b
 * takes tiles b, b + blocks, ... of its image. ---- */
constexpr size_t PLS_MAX_IMAGES = 65535;

inline size_t pls_grid_blocks(size_t n, uint64_t max_tiles)
{
    size_t blocks = (size_t)max_tiles;
    size_t cap = (2048 + n - 1) / n;
    if (cap < 8) cap = 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

/* rows of four pixels go through 16-byte loads when every cell row of both images starts on a 16-byte boundary: both bases do and the pitch is
 * a multiple of four pixels.  Otherwise word by word. */
PLS_HD bool pls_vector_rows(const void *a, const void *b, uint32_t width)
{
    return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) && !(width & 3u);
}

PLS_HD void pls_load4(uint32_t out[4], const uint32_t *row, bool vec)
{
    if (vec) {
        const PlsQuad q = *reinterpret_cast<const PlsQuad *>(row);
        out[0] = q.px[0]; out[1] = q.px[1]; out[2] = q.px[2]; out[3] = q.px[3];
    } else {
        out[0] = row[0]; out[1] = row[1]; out[2] = row[2]; out[3] = row[3];
    }
}

/* ---- visible mode (include/pngloss_hip.h, "Measuring over visible pixels"): the same arithmetic on the alpha-premultiplied pixels pm(a), pm(b) -- pm
 * keeps alpha and turns each of R, G, B into the integer nearest to c * A / 255, at most 255, so the PLS_*_MAX bounds hold as they stand -- and a
 * window counts only when one of its 64 pixels has a non-zero alpha in a or in b: when the alpha sums of its four cells, which the table holds
 * anyway, are not all zero. ---- */
PLS_HD uint32_t pls_pm(uint32_t p)
{
    const uint32_t A = p >> 24;
    return ((( p        & 255u) * A + 127u) / 255u) | ((((p >> 8) & 255u) * A + 127u) / 255u) << 8 | ((((p >> 16) & 255u) * A + 127u) / 255u) << 16 |
           (p & 0xFF000000u);
}

/* ---- the cells of a tile.  Thread `tid` of `nthreads` takes cells tid, tid + nthreads, ... of the tile's PLS_TILE_CELLS and writes the four
 * channels of each to table[cell * 4 + c].  A cell that is not wholly inside the image belongs to no window: it is not read and not written.
 * Visible: the sums are those of the premultiplied pixels. ---- */
template <bool Visible = false>
PLS_HD void pls_thread_cells(PlsCell *table, const uint32_t *a, const uint32_t *b, uint32_t width, uint32_t height, const PlsGeom &g, uint64_t tile,
                             uint32_t tid, uint32_t nthreads)
{
    const uint32_t tx = (uint32_t)(tile % g.tiles_x), ty = (uint32_t)(tile / g.tiles_x);
    const uint32_t ncx = width / PLS_CELL, ncy = height / PLS_CELL;
    const bool vec = pls_vector_rows(a, b, width);
    for (uint32_t cell = tid; cell < PLS_TILE_CELLS; cell += nthreads) {
        const uint32_t cx = tx * PLS_TILE_WX + cell % PLS_TILE_CX, cy = ty * PLS_TILE_WY + cell / PLS_TILE_CX;
        if (cx >= ncx || cy >= ncy) continue;
        uint32_t s[4] = {}, aa[4] = {}, bb[4] = {}, ab[4] = {};
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t r = 0; r < PLS_CELL; r++) {
            const size_t at = (size_t)(cy * PLS_CELL + r) * width + (size_t)cx * PLS_CELL;
            uint32_t pa[4], pb[4];
            pls_load4(pa, a + at, vec);
            pls_load4(pb, b + at, vec);
            if (Visible)
                for (int k = 0; k < 4; k++) { pa[k] = pls_pm(pa[k]); pb[k] = pls_pm(pb[k]); }
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; k++)
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int c = 0; c < 4; c++) {
                    const uint32_t va = (pa[k] >> (8 * c)) & 255u, vb = (pb[k] >> (8 * c)) & 255u;
                    s[c] += va | (vb << 16);
                    aa[c] += va * va;
                    bb[c] += vb * vb;
                    ab[c] += va * vb;
                }
        }
        for (int c = 0; c < 4; c++) table[cell * 4 + c] = PlsCell{ s[c], aa[c], bb[c], ab[c] };
    }
}

/* ---- the window arithmetic: q of one window and channel from its five sums ---- */
PLS_HD int32_t pls_q16(uint32_t sa, uint32_t sb, uint32_t saa, uint32_t sbb, uint32_t sab)
{
    const uint64_t m = (uint64_t)sa * sb, sq = (uint64_t)sa * sa + (uint64_t)sb * sb;
    const uint64_t a1 = 2 * m + PLS_K1, b1 = sq + PLS_K1;
    const int64_t a2 = 2 * ((int64_t)(64 * (uint64_t)sab) - (int64_t)m) + (int64_t)PLS_K2;
    const uint64_t b2 = 64 * ((uint64_t)saa + sbb) - sq + PLS_K2;
    const bool negative = a2 < 0;
    const uint64_t num = a1 * (uint64_t)(negative ? -a2 : a2), den = b1 * b2;       /* num <= den < 2^57, den > 0 */
    /* floor(num * 2^16 / den), and num * 2^16 does not fit 64 bits.  A double quotient is within 2^-36 of the true one (three roundings of 2^-53
     * on a value of at most 2^16), so its integer part e is the answer or one off it; which, the exact remainder num * 2^16 - e * den says.  That
     * remainder lies in [-den, 2 den) and den < 2^57, so it is exact in 64-bit arithmetic that wraps.  Integers in, an integer out: CPU and GPU
     * agree whatever their division rounds to.  (Two 64-bit divisions, or 16 rounds of shift and subtract, give the same value in some three times
     * the instructions: 64-bit division is emulated on gfx950, double division is not.) */
    uint32_t e = (uint32_t)((double)num * 65536.0 / (double)den);
    const int64_t rem = (int64_t)((num << 16) - (uint64_t)e * den);
    if (rem < 0) e--;
    else if (rem >= (int64_t)den) e++;
    return negative ? -(int32_t)e : (int32_t)e;
}

/* ---- the windows of a tile.  The partial record of a thread: its (window, channel) pairs tid, tid + nthreads, ... of the tile's PLS_TILE_ITEMS,
 * channel = pair % 4 -- so with nthreads a multiple of 4 a thread only ever sees channel tid % 4, and its record is that channel's. ---- */
struct PlsPart { int64_t sum; int32_t mn; uint32_t windows; };    /* windows: visible mode only, and only in the records of channel 3 */
PLS_HD PlsPart pls_part() { return PlsPart{ 0, PLS_ONE, 0 }; }

/* Visible: a window whose alpha sums (channel 3 of its four cells, both images) are all zero is skipped -- nothing added, no minimum lowered --
 * and the others are counted, once each: by the pair of channel 3. */
template <bool Visible = false>
PLS_HD void pls_thread_windows(PlsPart &p, const PlsCell *table, const PlsGeom &g, uint64_t tile, uint32_t tid, uint32_t nthreads)
{
    const uint32_t tx = (uint32_t)(tile % g.tiles_x), ty = (uint32_t)(tile / g.tiles_x);
    for (uint32_t item = tid; item < PLS_TILE_ITEMS; item += nthreads) {
        const uint32_t c = item & 3u, w = item >> 2, wx = w % PLS_TILE_WX, wy = w / PLS_TILE_WX;
        if (tx * PLS_TILE_WX + wx >= g.nx || ty * PLS_TILE_WY + wy >= g.ny) continue;
        const PlsCell *t = table + (size_t)(wy * PLS_TILE_CX + wx) * 4 + c;
        if (Visible) {
            const PlsCell *al = t + (3 - c);
            if (!(al[0].s | al[4].s | al[PLS_TILE_CX * 4].s | al[PLS_TILE_CX * 4 + 4].s)) continue;
            p.windows += c == 3 ? 1u : 0u;
        }
        const PlsCell c00 = t[0], c10 = t[4], c01 = t[PLS_TILE_CX * 4], c11 = t[PLS_TILE_CX * 4 + 4];
        const uint32_t s = c00.s + c10.s + c01.s + c11.s;              /* both halves stay below 2^16: 64 * 255 */
        const int32_t q = pls_q16(s & 0xFFFFu, s >> 16, c00.aa + c10.aa + c01.aa + c11.aa, c00.bb + c10.bb + c01.bb + c11.bb,
                                  c00.ab + c10.ab + c01.ab + c11.ab);
        p.sum += q;
        p.mn = q < p.mn ? q : p.mn;
    }
}

PLS_HD void pls_merge(PlsPart &p, const PlsPart &o)
{
    p.sum += o.sum;
    p.mn = o.mn < p.mn ? o.mn : p.mn;
    p.windows += o.windows;
}

/* the record before any window is added: what the launcher writes (the kernel adds to the sums and lowers the minima) */
inline PlSsimRecord pls_record_begin(uint32_t width, uint32_t height)
{
    return PlSsimRecord{ pls_geom(width, height).windows, { 0, 0, 0, 0 }, { PLS_ONE, PLS_ONE, PLS_ONE, PLS_ONE }, 0 };
}

/* ... in visible mode: the kernel counts the windows as well */
inline PlSsimRecord pls_record_begin_visible()
{
    return PlSsimRecord{ 0, { 0, 0, 0, 0 }, { PLS_ONE, PLS_ONE, PLS_ONE, PLS_ONE }, 0 };
}

/* Mean SSIM of a record over the channels of `channel_mask` (bit c = channel c): the one formula behind pngloss_hip_ssim_mean
 * (include/pngloss_hip.h says what it returns when) and behind the acceptance rule of pl_target.h.  Host arithmetic only. */
inline double pls_mean(uint64_t windows, const int64_t sum_q16[4], unsigned channel_mask)
{
    if (!windows || !channel_mask || channel_mask > 0xFu) return (double)NAN;
    int64_t sum = 0;
    int channels = 0;
    for (int c = 0; c < 4; c++)
        if (channel_mask & (1u << c)) { sum += sum_q16[c]; channels++; }
    return (double)sum / (65536.0 * (double)windows * (double)channels);
}

#endif

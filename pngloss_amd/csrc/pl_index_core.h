/*
 * pl_index_core.h -- the logic of the indexed-colour write side (option "indexed", include/pngloss_hip.h): count the distinct RGBA words of an
 * optimised image with an early exit past 256, order them into a palette, and turn the pixels into palette indices.  No reference equivalent (the
 * reference tool writes truecolour only).
 *
 * Definitions (all exact, restated with numpy in tests/util_index.py):
 *   colours        the distinct 32-bit words of the RGBA8 image (little-endian: R in the low byte, alpha in the high one)
 *   eligible       the image has pixels and 1 <= colours <= 256
 *   palette order  ascending by the word as a uint32: alpha most significant, then B, G, R -- entries that are not opaque come first, so the
 *                  tRNS chunk holds exactly the alphas of the first trns_entries entries
 *   index rows     colour type 3 at bit depth 8: per row a filter type byte 0 and `width` index bytes (depths 1 / 2 / 4: "the packed rows" below)
 *   decision       indexed is kept iff eligible and I + overhead < T (I, T: the complete zlib streams of the two encodings), a tie goes to truecolour;
 *                  overhead = 12 + 3 * entries + (trns_entries ? 12 + trns_entries : 0): the PLTE and tRNS chunks
 *
 * The table: PLI_SLOTS 64-bit slots per image, open addressing with linear probing, never more than PLI_SLOTS probes.  A slot is PLI_EMPTY (no
 * colour: its high half is not an index) or (index << 32) | word; while the colours are counted the high half is 0, pli_assign writes the palette
 * index there.  A colour is inserted with ONE compare-and-swap on the empty slot: of the threads that race for a slot exactly one wins, the others
 * see the winner's word in the value the swap returns and either find their own colour or probe on -- so the per-image counter, bumped by the
 * winner alone, is exact whatever the interleaving.  Nothing here waits for another thread.
 *
 * Shared by the HIP kernels (pl_index.hip) and by tests/c/index_host.cpp (test infrastructure), which runs the same bodies on the CPU under the
 * sanitizers, with one thread and with a team of threads that insert concurrently.
 */
#ifndef PL_INDEX_CORE_H
#define PL_INDEX_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLI_HD __host__ __device__ __forceinline__
#else
#define PLI_HD inline
#endif

constexpr uint32_t PLI_SLOTS = 1024;               /* per image; a power of two, four times the 257 insertions that decide */
constexpr uint32_t PLI_MAX_COLORS = 256;
constexpr uint32_t PLI_CACHE = 256;                /* a workgroup's pre-filter: 64-bit entries, PLI_EMPTY or a word this workgroup knows to be in the table */
constexpr uint64_t PLI_EMPTY = ~(uint64_t)0;
constexpr uint32_t PLI_QUAD = 4;                   /* pixels per thread and step: one 16-byte load, one dword of indices */

/* the three atomic accesses of the table and its counter: agent scope on the device (the workgroups of an image run on every XCD), the compiler's
 * builtins on the CPU */
#if defined(__HIP_DEVICE_COMPILE__)
#define PLI_LOAD64(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PLI_STORE64(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PLI_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PLI_ADD32(p, v) atomicAdd((p), (v))
PLI_HD uint64_t pli_cas64(uint64_t *p, uint64_t expect, uint64_t v)
{
    return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)expect, (unsigned long long)v);
}
#else
#define PLI_LOAD64(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define PLI_STORE64(p, v) __atomic_store_n((p), (v), __ATOMIC_RELAXED)
#define PLI_LOAD32(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define PLI_ADD32(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
PLI_HD uint64_t pli_cas64(uint64_t *p, uint64_t expect, uint64_t v)
{
    __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;                                  /* the value that was there: `expect` itself when the swap happened */
}
#endif

/* Fibonacci hashing: the top bits of word * 2^32 / phi */
PLI_HD uint32_t pli_mix(uint32_t word) { return word * 0x9E3779B1u; }
PLI_HD uint32_t pli_hash(uint32_t word) { return pli_mix(word) >> 22; }             /* 0 .. PLI_SLOTS - 1 */
PLI_HD uint32_t pli_cache_slot(uint32_t word) { return pli_mix(word) >> 24; }       /* 0 .. PLI_CACHE - 1 */
static_assert(PLI_SLOTS == 1u << 10 && PLI_CACHE == 1u << 8, "pli_hash and pli_cache_slot keep 10 and 8 bits");

/* 1: this call put the word into the table; 0: it was there; -1: given up -- PLI_SLOTS probes found neither the word nor room (the image has at
 * least PLI_SLOTS colours), or a long probe sequence found the counter past 256 on its way (a table of at most 256 colours is a quarter full and
 * its sequences are short; long ones belong to an image that is leaving anyway, and the counter is re-read every PLI_PROBE_CHECK probes so that
 * they end there) */
constexpr uint32_t PLI_PROBE_CHECK = 8;
PLI_HD int pli_insert(uint64_t *table, const uint32_t *count, uint32_t word)
{
    const uint32_t h = pli_hash(word);
    for (uint32_t k = 0; k < PLI_SLOTS; k++) {
        if (k && k % PLI_PROBE_CHECK == 0 && PLI_LOAD32(count) > PLI_MAX_COLORS) return -1;
        uint64_t *slot = table + ((h + k) & (PLI_SLOTS - 1));
        uint64_t cur = PLI_LOAD64(slot);
        if (cur == PLI_EMPTY) {
            cur = pli_cas64(slot, PLI_EMPTY, (uint64_t)word);
            if (cur == PLI_EMPTY) return 1;
        }
        if ((uint32_t)cur == word) return 0;
    }
    return -1;
}

/* one pixel word of the count: through the workgroup's pre-filter, then the table; the counter goes up with every insertion */
PLI_HD void pli_count_word(uint64_t *table, uint32_t *count, uint64_t *cache, uint32_t word)
{
    uint64_t *c = cache + pli_cache_slot(word);
    if (PLI_LOAD64(c) == (uint64_t)word) return;
    if (PLI_LOAD32(count) > PLI_MAX_COLORS) return;     /* decided: "more than 256" */
    const int r = pli_insert(table, count, word);
    if (r > 0) PLI_ADD32(count, 1u);
    if (r >= 0) PLI_STORE64(c, (uint64_t)word);     /* (only what IS in the table: an entry never hides a word that was not inserted) */
}

/* up to PLI_QUAD consecutive pixels: a word equal to the pixel before it was counted with that pixel (`before`: the pixel in front of w[0], any
 * value with has_before = false) */
PLI_HD void pli_count_quad(uint64_t *table, uint32_t *count, uint64_t *cache, const uint32_t *w, uint32_t m, bool has_before, uint32_t before)
{
    for (uint32_t k = 0; k < m; k++) {
        if (!(k ? w[k] == w[k - 1] : (has_before && w[0] == before))) pli_count_word(table, count, cache, w[k]);
    }
}

/* what the counter says once every workgroup is done: the number of colours, or 257 for "more than 256" */
PLI_HD uint32_t pli_colors_of(uint32_t count) { return count > PLI_MAX_COLORS ? PLI_MAX_COLORS + 1 : count; }

/* ---- the palette: the occupied slots gathered into a list (any order), every entry ranked among the others ---- */

/* the palette as the device leaves it: words[k] = entry k in palette order */
struct PliRecord {
    uint32_t entries, trns_entries;
    uint32_t words[PLI_MAX_COLORS];
};

/* slot `s` of the table into the list when it holds a colour; *m counts the entries (a list of PLI_MAX_COLORS: an entry beyond it is dropped) */
PLI_HD void pli_collect(const uint64_t *table, uint32_t s, uint32_t *list_word, uint32_t *list_slot, uint32_t *m)
{
    const uint64_t cur = table[s];
    if (cur == PLI_EMPTY) return;
    const uint32_t k = PLI_ADD32(m, 1u);
    if (k < PLI_MAX_COLORS) { list_word[k] = (uint32_t)cur; list_slot[k] = s; }
}

/* entry k of a list of m distinct words: its place in ascending order */
PLI_HD uint32_t pli_rank(const uint32_t *list_word, uint32_t m, uint32_t k)
{
    uint32_t rank = 0;
    for (uint32_t i = 0; i < m; i++) rank += list_word[i] < list_word[k] ? 1u : 0u;
    return rank;
}

/* ... written into the record and beside the colour in its slot (rec->trns_entries: zero before the first call) */
PLI_HD void pli_assign(uint64_t *table, const uint32_t *list_word, const uint32_t *list_slot, uint32_t m, uint32_t k, PliRecord *rec)
{
    const uint32_t rank = pli_rank(list_word, m, k), word = list_word[k];
    rec->words[rank] = word;
    table[list_slot[k]] = ((uint64_t)rank << 32) | word;
    if ((word >> 24) != 255u) PLI_ADD32(&rec->trns_entries, 1u);
}

/* ---- the index rows ---- */

/* the palette index of a word (0 for a word the table does not hold: cannot happen for a pixel of the image the table was built from) */
PLI_HD uint32_t pli_lookup(const uint64_t *table, uint32_t word)
{
    const uint32_t h = pli_hash(word);
    for (uint32_t k = 0; k < PLI_SLOTS; k++) {
        const uint64_t cur = table[(h + k) & (PLI_SLOTS - 1)];
        if (cur == PLI_EMPTY) return 0;
        if ((uint32_t)cur == word) return (uint32_t)(cur >> 32);
    }
    return 0;
}

/* m <= PLI_QUAD pixels into one dword of index bytes, pixel 0 in the low byte; the bytes behind the row's last pixel are 0 */
PLI_HD uint32_t pli_pack_quad(const uint64_t *table, const uint32_t *w, uint32_t m)
{
    uint32_t out = 0, idx = 0;
    for (uint32_t k = 0; k < m; k++) {
        if (!k || w[k] != w[k - 1]) idx = pli_lookup(table, w[k]);
        out |= idx << (8 * k);
    }
    return out;
}

/* ---- the decision (host arithmetic) ---- */

inline uint64_t pli_overhead(uint32_t entries, uint32_t trns_entries) { return 12u + 3u * (uint64_t)entries + (trns_entries ? 12u + trns_entries : 0u); }
inline bool pli_keep_indexed(uint32_t colors, uint64_t indexed_bytes, uint64_t truecolor_bytes, uint32_t trns_entries)
{
    return colors >= 1 && colors <= PLI_MAX_COLORS && indexed_bytes + pli_overhead(colors, trns_entries) < truecolor_bytes;
}

/* ---- the packed rows: bit depths 1, 2 and 4 (option "index_depth", include/pngloss_hip_index_depth.h; restated with numpy in
 * tests/util_index_depth.py) ----
 *   min_depth(entries)  1 for 1..2 entries, 2 for 3..4, 4 for 5..16, 8 for 17..256 (0 for anything else: no palette)
 *   packed scanline at depth d in {1, 2, 4}: the filter type byte 0, then ceil(width * d / 8) bytes; pixel x lies in byte x * d / 8 at the shift
 *                       8 - d * (x % (8 / d) + 1) -- the leftmost pixel in the high bits, as PNG requires; the unused low bits of a row's last byte are 0
 *   the palette, its order, tRNS and the overhead are the ones above, unchanged
 * The packed rows are made from the 8-bit index rows pl_index_rows has written, not from the pixels: one thread makes one dword of a packed row, in
 * memory order (first byte low), from 32 / 16 / 8 index bytes at depth 1 / 2 / 4.  Of an 8-bit row only the bytes up to its last dword are written,
 * and only `width` of them are indices: everything behind `width` is masked here, never trusted. */

PLI_HD uint32_t pli_min_depth(uint32_t entries)
{
    return entries < 1 || entries > PLI_MAX_COLORS ? 0u : entries <= 2 ? 1u : entries <= 4 ? 2u : entries <= 16 ? 4u : 8u;
}

/* four index bytes (pixel 0 in the low byte) as 4 * D bits of a packed row.  D = 1: a nibble, pixel 0 its high bit; D = 2: a byte, pixel 0 its
 * high two bits -- the multiplications move every masked field to a place of its own, so nothing carries; D = 4: two bytes, the first one low */
template <uint32_t D> PLI_HD uint32_t pli_pack_word(uint32_t w)
{
    static_assert(D == 1 || D == 2 || D == 4, "the packed depths");
    if (D == 1) return ((w & 0x01010101u) * 0x80402010u) >> 28;
    if (D == 2) return ((w & 0x03030303u) * 0x40100401u) >> 24;
    const uint32_t t = w & 0x0F0F0F0Fu, u = (t << 4) | (t >> 8);
    return (u & 0xFFu) | ((u >> 8) & 0xFF00u);
}

/* one dword of a packed row from the 32 / D index bytes in src[0 .. 8 / D): the first `valid` of them are pixels of the row, the others are masked */
template <uint32_t D> PLI_HD uint32_t pli_pack_dword(const uint32_t *src, uint32_t valid)
{
    uint32_t out = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 8 / D; k++) {
        const uint32_t m = valid > 4 * k ? valid - 4 * k : 0u;
        const uint32_t keep = m >= 4 ? ~0u : (1u << (8 * m)) - 1u;
        out |= pli_pack_word<D>(src[k] & keep) << (D == 1 ? 8 * (k >> 1) + 4 * (1 - (k & 1)) : 4 * D * k);
    }
    return out;
}

/* dword q of the packed row of the 8-bit row `row8` (16-byte aligned, its pitch a multiple of 16 and >= width; q * 32 / D < width).  The index bytes
 * come in 16-byte loads (8 at depth 4).  At depth 1 a thread has two of them, and the second may start behind the row's pitch -- the pitch is a
 * multiple of 16, not of 32 --, so a load that starts at or behind `width` is left out: one that starts in front of it ends inside the pitch. */
template <uint32_t D> PLI_HD uint32_t pli_pack_lane(const uint8_t *row8, uint32_t width, uint32_t q)
{
    constexpr uint32_t per = 32 / D, words = 8 / D, step = words < 4 ? words : 4;      /* dwords a load brings */
    const uint32_t x = q * per, valid = width - x < per ? width - x : per;
    uint32_t src[words];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t g = 0; g < words; g += step) {
        if (x + 4 * g < width) __builtin_memcpy(src + g, __builtin_assume_aligned(row8 + x + 4 * g, 4 * step), 4 * step);
        else for (uint32_t k = 0; k < step; k++) src[g + k] = 0u;
    }
    return pli_pack_dword<D>(src, valid);
}

/* ... with the depth as a value */
PLI_HD uint32_t pli_pack_lane_at(uint32_t depth, const uint8_t *row8, uint32_t width, uint32_t q)
{
    return depth == 1 ? pli_pack_lane<1>(row8, width, q) : depth == 2 ? pli_pack_lane<2>(row8, width, q) : pli_pack_lane<4>(row8, width, q);
}

/* dwords of a packed row that hold pixels, and its bytes as the deflate reads them */
PLI_HD uint32_t pli_packed_dwords(uint32_t width, uint32_t depth) { return (uint32_t)(((uint64_t)width * depth + 31) / 32); }
PLI_HD uint32_t pli_packed_rowbytes(uint32_t width, uint32_t depth) { return (uint32_t)(((uint64_t)width * depth + 7) / 8); }

/* ---- which stream is kept under the option "index_depth" (host arithmetic; pli_keep_indexed above is the rule of "8") ----
 *   candidates  T: the truecolour stream; I8: the 8-bit index rows; Ip: the rows packed at min_depth, for an eligible image with min_depth < 8
 *   "8"         T against I8
 *   "auto"      the smallest of T, I8 + overhead, Ip + overhead; a tie goes to the earlier one in that order
 *   "min"       T against the indexed stream at min_depth alone (for 17..256 colours that is I8) */
enum PliDepthMode : uint32_t { PLI_DEPTH_8 = 0, PLI_DEPTH_AUTO = 1, PLI_DEPTH_MIN = 2 };

/* which indexed candidates an image of `colors` colours (257: more than 256) gets */
inline bool pli_wants_packed(uint32_t mode, uint32_t colors) { return mode != PLI_DEPTH_8 && pli_min_depth(colors) >= 1 && pli_min_depth(colors) < 8; }
inline bool pli_wants_indexed8(uint32_t mode, uint32_t colors) { return pli_min_depth(colors) >= 1 && (mode != PLI_DEPTH_MIN || pli_min_depth(colors) == 8); }

/* the bit depth of the stream that is kept; 0: truecolour.  The size of a candidate the image did not get is not read. */
inline uint32_t pli_keep_depth(uint32_t mode, uint32_t colors, uint64_t indexed8_bytes, uint64_t packed_bytes, uint64_t truecolor_bytes, uint32_t trns_entries)
{
    uint64_t best = truecolor_bytes;
    uint32_t depth = 0;
    const uint64_t overhead = pli_overhead(colors, trns_entries);
    if (pli_wants_indexed8(mode, colors) && indexed8_bytes + overhead < best) { best = indexed8_bytes + overhead; depth = 8; }
    if (pli_wants_packed(mode, colors) && packed_bytes + overhead < best) depth = pli_min_depth(colors);
    return depth;
}

/* the indexed candidate that was compared with T (pngloss_hip_palette.indexed_bytes): the smaller one where there are two; 0 when not eligible */
inline uint64_t pli_indexed_candidate(uint32_t mode, uint32_t colors, uint64_t indexed8_bytes, uint64_t packed_bytes)
{
    if (!pli_wants_packed(mode, colors)) return pli_wants_indexed8(mode, colors) ? indexed8_bytes : 0u;
    if (!pli_wants_indexed8(mode, colors)) return packed_bytes;
    return packed_bytes < indexed8_bytes ? packed_bytes : indexed8_bytes;
}

#endif

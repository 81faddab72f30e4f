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
 *   index rows     colour type 3 at bit depth 8: per row a filter type byte 0 and `width` index bytes (depths 1 / 2 / 4 are not written)
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

#endif

/*
 * pl_size.h -- the decisions of pngloss_hip_optimize_batch_size: a strength per image, found from a byte budget for its zlib stream.  No reference
 * equivalent (the reference tool takes a strength and reports the size it got).
 *
 * Plain C++ without HIP types, like pl_target.h, whose search this mirrors in the other direction: everything the search DECIDES is here, so that
 * tests/c/size_host.cpp drives it on the CPU.  pl_search.h keeps the books of a whole search on top of these functions (what is kept, which
 * regions are copied where), and pl_host_search.hip does what the two say: it runs the groups through enqueue() / finish() with emit descriptors,
 * measures the emitted scanlines with pl_deflate_measure and carries out the moves with pl_move.
 *
 * A probe is ACCEPTED when its status is 0 and its stream -- the complete zlib stream, 78 DA ... Adler-32 -- has at most max_bytes bytes.
 * The size is not guaranteed to be monotone in the strength, so the result is defined by this procedure, per image (include/pngloss_hip.h states
 * it for callers), with M = max_strength:
 *   1. probe M; refused: the chosen strength is M and reached = 0 (the image keeps the M result)
 *   2. else lo = -1 (virtual, refused), hi = M
 *   3. while hi - lo > 1: probe mid = floor((lo + hi) / 2); accepted: hi = mid, else lo = mid
 *   4. the chosen strength is hi, reached = 1
 * At most 1 + ceil(log2(M + 1)) probes.  Strength 0 is probed only when every probe above it passed: the lossless file, when it already fits.
 * A probe whose status is not 0 ends the search: the image keeps that probe's result.  An image without pixels is chosen 0 with 0 probes.
 */
#ifndef PL_SIZE_H
#define PL_SIZE_H

#include "../../include/pngloss_hip.h"
#include "pl_target.h"

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

constexpr uint64_t PL_SIZE_MAX_SCANLINES = 1ull << 30;     /* PL_DEFLATE_MAX_STREAM: the deflate's positions are 32-bit */

/* PNGLOSS_SUCCESS, or PNGLOSS_INVALID_ARGUMENT for what the header rules out: no target, M above 255, no budget or a budget of 0 for an image
 * that has pixels, an image beyond the deflate's 1 GiB of scanlines.  Looked at before any image is touched. */
inline int pl_size_check(const pngloss_hip_size_target *t, size_t n, const uint32_t *width, const uint32_t *height)
{
    if (!t || t->max_strength > 255u) return PNGLOSS_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; i++) {
        if (!width[i] || !height[i]) continue;
        if (!t->max_bytes || t->max_bytes[i] == 0) return PNGLOSS_INVALID_ARGUMENT;
        if (((uint64_t)width[i] * 4 + 1) * height[i] > PL_SIZE_MAX_SCANLINES) return PNGLOSS_INVALID_ARGUMENT;
    }
    return PNGLOSS_SUCCESS;
}

inline bool pl_size_accept(int32_t status, uint64_t stream_bytes, uint64_t max_bytes) { return status == 0 && stream_bytes <= max_bytes; }

/* The search of one image.  While !done, `next` is the strength to probe; pl_size_step takes that probe's verdict. */
struct PlSizeSearch {
    long lo = -1;
    uint32_t hi = 0;
    uint32_t next = 0;
    uint32_t probes = 0;
    uint32_t chosen = 0;
    uint32_t reached = 0;           /* the chosen strength's stream is within the budget */
    bool first = true, done = false;
    bool failed = false;            /* ended by a probe whose status was not 0: chosen = that probe's strength */
};

inline PlSizeSearch pl_size_begin(uint32_t max_strength, bool has_pixels)
{
    PlSizeSearch s;
    s.next = max_strength;
    if (!has_pixels) { s.done = true; s.first = false; s.reached = 1; }      /* nothing to write: chosen 0, no probe */
    return s;
}

inline void pl_size_step(PlSizeSearch &s, bool accepted)
{
    if (s.done) return;
    s.probes++;
    if (s.first) {
        s.first = false;
        if (!accepted) { s.chosen = s.next; s.reached = 0; s.done = true; return; }
        s.lo = -1; s.hi = s.next;
    } else if (accepted) s.hi = s.next;
    else s.lo = (long)s.next;
    if ((long)s.hi - s.lo > 1) s.next = (uint32_t)((s.lo + (long)s.hi) / 2);      /* (the sum is >= 0 here: floor and truncation agree) */
    else { s.chosen = s.hi; s.reached = 1; s.done = true; }
}

/* the probe of s.next came back with a status other than 0 */
inline void pl_size_fail(PlSizeSearch &s)
{
    if (s.done) return;
    s.probes++;
    s.chosen = s.next;
    s.reached = 0;
    s.first = false; s.done = true; s.failed = true;
}

/* the most probes a search below M can take: 1 + ceil(log2(M + 1)) */
inline uint32_t pl_size_probe_bound(uint32_t max_strength)
{
    uint32_t b = 1;
    for (uint32_t span = 1; span < max_strength + 1u; span *= 2) b++;
    return b;
}

/* One round: pl_search_groups (pl_target.h) over the size searches, under the name tests/c/size_host.cpp pins it */
inline std::vector<std::pair<uint32_t, std::vector<uint32_t>>> pl_size_groups(const std::vector<PlSizeSearch> &s) { return pl_search_groups(s); }

#endif

/*
 * pl_target.h -- the decisions of pngloss_hip_optimize_batch_target: a strength per image, found from a distortion target.  No reference equivalent
 * (the reference tool takes a strength and reports file sizes only).
 *
 * Plain C++ without HIP types, like pl_plan.h: everything the search DECIDES is here -- whether a target is valid, whether a probe is accepted,
 * which strength an image probes next and which one it ends with, which images of a round share a batch, and where the search arena keeps what --
 * so that tests/c/target_host.cpp drives it on the CPU.  pl_search.h keeps the books of a whole search on top of these functions (what is kept,
 * which regions are copied where), and pl_host_search.hip does what the two say: it runs the groups through enqueue() / finish(), measures with
 * pl_distort and carries out the moves with pl_move (pl_target.hip).
 *
 * The rule, per image (include/pngloss_hip.h states it for callers).  PSNR is not monotone in the strength, so the result is defined by this
 * procedure and not by "the largest strength that passes":
 *   1. probe M = max_strength; accepted: the chosen strength is M
 *   2. else lo = 0, hi = M (strength 0 changes no pixel and counts as accepted without a probe)
 *   3. while hi - lo > 1: probe mid = (lo + hi) / 2; accepted: lo = mid, else hi = mid
 *   4. the chosen strength is lo
 * At most 1 + ceil(log2 M) probes, 1 for M <= 1.  A probe whose status is not 0 ends the search: the image keeps that probe's result.
 *
 * pngloss_hip_optimize_batch_target2 adds a smallest mean SSIM to the target (pngloss_hip_target2): the same procedure, one more condition in the
 * acceptance rule (pl_target_accept2), one more record table in the arena.  The older target is the newer one with min_ssim = 0.
 */
#ifndef PL_TARGET_H
#define PL_TARGET_H

#include "../../include/pngloss_hip.h"
#include "pl_distort_core.h"
#include "pl_ssim_core.h"

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

/* PNGLOSS_SUCCESS, or PNGLOSS_INVALID_ARGUMENT for a target the header rules out */
inline int pl_target_check(const pngloss_hip_target *t)
{
    if (!t) return PNGLOSS_INVALID_ARGUMENT;
    if (t->min_psnr_db != t->min_psnr_db || t->min_psnr_db < 0.0) return PNGLOSS_INVALID_ARGUMENT;      /* NaN, negative */
    if (t->max_abs_error > 255u || t->max_strength > 255u) return PNGLOSS_INVALID_ARGUMENT;
    return PNGLOSS_SUCCESS;
}

/* the older target as the newer one: no SSIM condition */
inline pngloss_hip_target2 pl_target2_of(const pngloss_hip_target &t)
{
    return pngloss_hip_target2{ t.min_psnr_db, t.max_abs_error, t.max_strength, 0.0 };
}

/* the same for a pngloss_hip_target2: min_ssim is 0 (no condition) or in (0, 1] */
inline int pl_target_check2(const pngloss_hip_target2 *t)
{
    if (!t) return PNGLOSS_INVALID_ARGUMENT;
    const pngloss_hip_target old = { t->min_psnr_db, t->max_abs_error, t->max_strength };
    if (pl_target_check(&old) != PNGLOSS_SUCCESS) return PNGLOSS_INVALID_ARGUMENT;
    if (t->min_ssim != t->min_ssim || t->min_ssim < 0.0 || t->min_ssim > 1.0) return PNGLOSS_INVALID_ARGUMENT;   /* NaN, negative, above 1 */
    return PNGLOSS_SUCCESS;
}

/* the channels an image of 1 / 2 / 3 / 4 bytes per pixel stores (gray is the G channel): the mask `pngloss --distortion` prints with */
inline unsigned pl_target_mask_of_bpp(uint32_t bytes_per_pixel)
{
    return bytes_per_pixel == 1 ? 0x2u : bytes_per_pixel == 2 ? 0xAu : bytes_per_pixel == 3 ? 0x7u : 0xFu;
}

/* Is a probe accepted: `rec` is the probed result against its original, status / bytes_per_pixel those of the probe's pngloss_hip_result */
inline bool pl_target_accept(const pngloss_hip_target &t, const pngloss_hip_distortion &rec, int32_t status, uint32_t bytes_per_pixel)
{
    if (status != 0) return false;
    if (!rec.pixels) return true;                                 /* an image without pixels */
    const unsigned mask = pl_target_mask_of_bpp(bytes_per_pixel);
    if (t.min_psnr_db != 0.0 && !(pld_psnr_db(rec.pixels, rec.sq_err, mask) >= t.min_psnr_db)) return false;
    if (t.max_abs_error) {
        uint32_t largest = 0;
        for (int c = 0; c < 4; c++)
            if ((mask >> c & 1u) && rec.max_abs[c] > largest) largest = rec.max_abs[c];
        if (largest > t.max_abs_error) return false;
    }
    return true;
}

/* The same with the SSIM condition: `srec` is the probe's SSIM record (not looked at when min_ssim == 0).  An image without windows -- narrower or
 * lower than 8 pixels -- cannot be measured: the condition does not apply to it. */
inline bool pl_target_accept2(const pngloss_hip_target2 &t, const pngloss_hip_distortion &rec, const pngloss_hip_ssim &srec, int32_t status, uint32_t bytes_per_pixel)
{
    const pngloss_hip_target old = { t.min_psnr_db, t.max_abs_error, t.max_strength };
    if (!pl_target_accept(old, rec, status, bytes_per_pixel)) return false;
    if (t.min_ssim == 0.0 || !rec.pixels || !srec.windows) return true;
    return pls_mean(srec.windows, srec.sum_q16, pl_target_mask_of_bpp(bytes_per_pixel)) >= t.min_ssim;
}

/* The search of one image.  While !done, `next` is the strength to probe; pl_target_step takes that probe's verdict. */
struct PlTargetSearch {
    uint32_t lo = 0, hi = 0;
    uint32_t next = 0;
    uint32_t probes = 0;
    uint32_t chosen = 0;
    bool first = true, done = false;
    bool failed = false;            /* ended by a probe whose status was not 0: chosen = that probe's strength */
};

inline PlTargetSearch pl_target_begin(uint32_t max_strength)
{
    PlTargetSearch s;
    s.next = max_strength;
    return s;
}

inline void pl_target_step(PlTargetSearch &s, bool accepted)
{
    if (s.done) return;
    s.probes++;
    if (s.first) {
        s.first = false;
        if (accepted) { s.chosen = s.next; s.done = true; return; }
        s.lo = 0; s.hi = s.next;
    } else if (accepted) s.lo = s.next;
    else s.hi = s.next;
    if (s.hi - s.lo > 1) s.next = (s.lo + s.hi) / 2;
    else { s.chosen = s.lo; s.done = true; }
}

/* the probe of s.next came back with a status other than 0 */
inline void pl_target_fail(PlTargetSearch &s)
{
    if (s.done) return;
    s.probes++;
    s.chosen = s.next;
    s.first = false; s.done = true; s.failed = true;
}

/* the most probes a search below M can take: 1 + ceil(log2 M), 1 for M <= 1 */
inline uint32_t pl_target_probe_bound(uint32_t max_strength)
{
    uint32_t b = 1;
    for (uint32_t span = 1; span < max_strength; span *= 2) b++;
    return b;
}

/* One round of either search: the images still searching, grouped by the strength they probe next -- ascending strengths, images in input order.
 * Each group runs as one ordinary batch.  Search: PlTargetSearch or PlSizeSearch (pl_size.h); pl_search.h begins every round with it. */
template <class Search>
inline std::vector<std::pair<uint32_t, std::vector<uint32_t>>> pl_search_groups(const std::vector<Search> &s)
{
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> out;
    for (uint32_t strength = 0; strength < 256; strength++) {
        std::vector<uint32_t> who;
        for (size_t i = 0; i < s.size(); i++)
            if (!s[i].done && s[i].next == strength) who.push_back((uint32_t)i);
        if (!who.empty()) out.emplace_back(strength, std::move(who));
    }
    return out;
}
/* (the name tests/c/target_host.cpp pins it under) */
inline std::vector<std::pair<uint32_t, std::vector<uint32_t>>> pl_target_groups(const std::vector<PlTargetSearch> &s) { return pl_search_groups(s); }

/* ---- the search arena of a context: apart from the workspace and from the keep arena of the option "distortion" (every enqueue() lays that one
 * out afresh, which would lose the originals of the images outside the current group).  In front the tables -- the move jobs of one launch (at
 * most three per image: pixels, filters, and pixels of another kind in the last launch), the measuring jobs and their records, with an SSIM
 * condition also the SSIM kernel's jobs and records --, behind them per
 * image its original, the best result so far and that result's row filters; for host images also the image itself and its filters.  The size search
 * (pl_size.h) asks for one more region per image, `scanlines`: the rows pl_emit writes for a probe -- height rows of `pitch` bytes, the pitch
 * pl_window_layout gives emitted rows (4 * width rounded up to 16: pl_emit stores whole 16-byte groups) -- and the row's filter ids, height
 * bytes; PLT_SCANLINES_PROBE_AND_BEST adds the same again for the best result so far.  Without it the layout is what it was before the region existed. */
constexpr size_t PLT_ALIGN = 256;
constexpr size_t PLT_MOVES_PER_IMAGE = 3;
constexpr size_t PLT_SIZE_MOVES_PER_IMAGE = 4;     /* the size search stashes pixels, filters, rows and ids of an accepted probe in one launch */
constexpr int PLT_SCANLINES_OFF = 0, PLT_SCANLINES_PROBE = 1, PLT_SCANLINES_PROBE_AND_BEST = 2;
struct PlTargetImage {
    size_t orig = 0, best = 0, best_filters = 0, img = 0, filters = 0;
    size_t rows = 0, ids = 0;       /* with `scanlines`: the emitted rows and their filter ids */
    size_t best_rows = 0, best_ids = 0;     /* PLT_SCANLINES_PROBE_AND_BEST: those of the best result so far (the caller wants its stream written) */
    uint32_t pitch = 0;             /* ... and the rows' pitch; 0: the image has no pixels, nothing is emitted */
};
struct PlTargetLayout {
    size_t moves = 0, jobs = 0, records = 0, total = 0;
    size_t ssim_jobs = 0, ssim_records = 0;        /* the SSIM kernel's job table and records (no bytes when the search has no SSIM condition) */
    size_t flags = 0;                              /* with `scanlines`: one out-flags word per image, gathered by pl_move so that ONE copy brings a group's to the host */
    std::vector<PlTargetImage> image;
};

inline PlTargetLayout pl_target_layout(const std::vector<uint32_t> &width, const std::vector<uint32_t> &height, bool host_images,
                                       size_t move_job_bytes, size_t distort_job_bytes, size_t record_bytes,
                                       size_t ssim_job_bytes = 0, size_t ssim_record_bytes = 0, int scanlines = PLT_SCANLINES_OFF)
{
    auto up = [](size_t v) { return (v + PLT_ALIGN - 1) / PLT_ALIGN * PLT_ALIGN; };
    const size_t n = width.size();
    PlTargetLayout lay;
    size_t at = 0;
    lay.moves = at; at = up(at + move_job_bytes * (scanlines ? PLT_SIZE_MOVES_PER_IMAGE : PLT_MOVES_PER_IMAGE) * n);
    lay.jobs = at; at = up(at + distort_job_bytes * n);
    lay.records = at; at = up(at + record_bytes * n);
    lay.ssim_jobs = at; at = up(at + ssim_job_bytes * n);
    lay.ssim_records = at; at = up(at + ssim_record_bytes * n);
    if (scanlines) { lay.flags = at; at = up(at + sizeof(uint32_t) * n); }
    lay.image.resize(n);
    for (size_t i = 0; i < n; i++) {
        const size_t px = (size_t)width[i] * height[i] * 4, rows = width[i] ? height[i] : 0;
        PlTargetImage &m = lay.image[i];
        m.orig = at; at = up(at + px);
        m.best = at; at = up(at + px);
        m.best_filters = at; at = up(at + rows);
        if (host_images) {
            m.img = at; at = up(at + px);
            m.filters = at; at = up(at + rows);
        }
        if (scanlines) {
            m.pitch = px ? (uint32_t)(((size_t)width[i] * 4 + 15) / 16 * 16) : 0;
            m.rows = at; at = up(at + (size_t)m.pitch * height[i]);
            m.ids = at; at = up(at + (m.pitch ? height[i] : 0));
            if (scanlines == PLT_SCANLINES_PROBE_AND_BEST) {
                m.best_rows = at; at = up(at + (size_t)m.pitch * height[i]);
                m.best_ids = at; at = up(at + (m.pitch ? height[i] : 0));
            }
        }
    }
    lay.total = at;
    return lay;
}

#endif

/*
 * pl_search.h -- the bookkeeping of the two strength searches (pl_target.h: from a distortion target, pl_size.h: from a byte budget): per image
 * what the last probe gave, what is kept, which strength's result lies where in the search arena -- and, from that, which regions a round copies
 * where.  Internal.
 *
 * Plain C++ without HIP types, like pl_target.h and pl_size.h: the copies are SYMBOLIC here (image, source region, destination region), so that
 * tests/c/search_host.cpp simulates the device with a tag per region and drives whole searches on the CPU (tests/test_search_host.py).
 * pl_host_search.hip:target_search / size_search call these functions for every decision, turn the moves into pl_move jobs (one table = one launch) and
 * do the device work in between: the batches, the measurements, the reports.
 *
 * What the functions keep true:
 *   - every probe of an image starts from its original (PLA_ORIG, saved by pl_search_open and copied back by the round when the image holds a result)
 *   - an accepted probe that is not the image's last one is stashed (PLA_BEST, PLA_BEST_FILTERS; the size search that writes streams also stashes
 *     the emitted rows and ids), so that the close can put it back when a later probe was refused
 *   - a table never has more moves than the layout reserves per image (PLT_MOVES_PER_IMAGE, PLT_SIZE_MOVES_PER_IMAGE), no two with one
 *     destination, none that reads what another one writes
 *   - an image whose probe failed (status other than 0) keeps that probe: record kept, result in place, nothing moved afterwards
 */
#ifndef PL_SEARCH_H
#define PL_SEARCH_H

#include "pl_target.h"
#include "pl_size.h"
#include "pl_layout.h"

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

/* the places a search copies between: the caller's image and its row filters, and the regions of PlTargetImage */
enum PlArenaRegion : uint8_t { PLA_IMAGE, PLA_FILTERS, PLA_ORIG, PLA_BEST, PLA_BEST_FILTERS, PLA_ROWS, PLA_IDS, PLA_BEST_ROWS, PLA_BEST_IDS, PLA_REGIONS };

struct PlSearchMove {
    uint32_t image;
    PlArenaRegion src, dst;
};

/* the bytes a region of one image holds: pixels; a filter id per row where the image has a width and a filter array; the emitted rows and their
 * ids where the layout gave the image a pitch.  A move of 0 bytes is no job. */
inline uint64_t pl_search_region_bytes(PlArenaRegion r, uint32_t width, uint32_t height, bool has_filters, uint32_t pitch)
{
    switch (r) {
    case PLA_IMAGE: case PLA_ORIG: case PLA_BEST: return (uint64_t)width * height * 4;
    case PLA_FILTERS: case PLA_BEST_FILTERS: return (width && has_filters) ? height : 0;
    case PLA_ROWS: case PLA_BEST_ROWS: return (uint64_t)pitch * height;
    case PLA_IDS: case PLA_BEST_IDS: return pitch ? height : 0;
    default: return 0;
    }
}

/* what a probe gave: the batch's result and what the search measured on it */
struct PlTargetProbe {
    pngloss_hip_result result{};
    pngloss_hip_distortion rec{};
    pngloss_hip_ssim ssim{};            /* (only with an SSIM condition) */
};
struct PlSizeProbe {
    pngloss_hip_result result{};
    uint32_t flags = 0;                 /* the out-flags word: colour type and bytes per pixel of the scanlines */
    PlSizeRecord size{};                /* the measured stream */
};

/* One image of a search */
template <class Search, class Probe>
struct PlSearchTrack {
    Search search;
    Probe last{}, kept{};               /* of the probe just run / of the result the image ends with */
    long best = -1;                     /* the strength whose (accepted) result the arena's stash holds; -1: none */
    long in_place = -1;                 /* the strength whose result the image itself holds; -1: the original */
    bool kept_in_stash = false;         /* size search: the kept result's scanlines are the stash's (else the probe region's) */
    uint32_t runs = 0;
};
using PlTargetTrack = PlSearchTrack<PlTargetSearch, PlTargetProbe>;
using PlSizeTrack = PlSearchTrack<PlSizeSearch, PlSizeProbe>;

/* Open: the originals, before the first probe rewrites the images in place */
inline std::vector<PlSearchMove> pl_search_open(size_t n)
{
    std::vector<PlSearchMove> save;
    for (size_t i = 0; i < n; i++) save.push_back(PlSearchMove{ (uint32_t)i, PLA_IMAGE, PLA_ORIG });
    return save;
}

/* Begin a round: its groups (none: the search is over), the originals back into the probed images that hold a result, and the probed images in
 * the order of the groups */
struct PlSearchRound {
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> groups;
    std::vector<PlSearchMove> back;
    std::vector<uint32_t> probed;
};
template <class Track>
inline PlSearchRound pl_search_round(const std::vector<Track> &st)
{
    std::vector<decltype(Track::search)> searches(st.size());
    for (size_t i = 0; i < st.size(); i++) searches[i] = st[i].search;
    PlSearchRound r;
    r.groups = pl_search_groups(searches);
    for (const auto &g : r.groups)
        for (uint32_t i : g.second) {
            if (st[i].in_place >= 0) r.back.push_back(PlSearchMove{ i, PLA_ORIG, PLA_IMAGE });
            r.probed.push_back(i);
        }
    return r;
}

/* A probe ran: the image holds the result of `strength` */
template <class Track>
inline void pl_search_ran(Track &s, uint32_t strength, const pngloss_hip_result &result)
{
    s.last.result = result;
    s.in_place = (long)strength;
    s.runs++;
}

/* Settle the probes of a round, target rule: every image of `probed` has its `last` complete.  Returns the moves that stash the accepted probes
 * whose images search on. */
inline std::vector<PlSearchMove> pl_target_settle(std::vector<PlTargetTrack> &st, const std::vector<uint32_t> &probed, const pngloss_hip_target2 &t)
{
    std::vector<PlSearchMove> stash;
    for (uint32_t i : probed) {
        PlTargetTrack &s = st[i];
        if (s.last.result.status != 0) {                     /* ends this image's search: it keeps this probe's result and status */
            pl_target_fail(s.search);
            s.kept = s.last;
            continue;
        }
        const bool accepted = pl_target_accept2(t, s.last.rec, s.last.ssim, s.last.result.status, s.last.result.bytes_per_pixel);
        const uint32_t strength = s.search.next;
        pl_target_step(s.search, accepted);
        if (!accepted) continue;
        s.kept = s.last; s.best = (long)strength;
        if (s.search.done) continue;                         /* (the chosen strength's result is in place) */
        stash.push_back(PlSearchMove{ i, PLA_IMAGE, PLA_BEST });
        stash.push_back(PlSearchMove{ i, PLA_FILTERS, PLA_BEST_FILTERS });
    }
    return stash;
}

/* The same, size rule: max_bytes[i] is the budget of image i.  want_streams: the stash also takes the emitted rows and ids. */
inline std::vector<PlSearchMove> pl_size_settle(std::vector<PlSizeTrack> &st, const std::vector<uint32_t> &probed, const uint64_t *max_bytes, bool want_streams)
{
    std::vector<PlSearchMove> stash;
    for (uint32_t i : probed) {
        PlSizeTrack &s = st[i];
        if (s.last.result.status != 0) {                     /* ends this image's search: it keeps this probe's result and status */
            pl_size_fail(s.search);
            s.kept = s.last; s.kept.flags = 0; s.kept.size = PlSizeRecord{ 0, 1, { 0, 0, 0 } }; s.kept_in_stash = false;
            continue;
        }
        const bool accepted = pl_size_accept(s.last.result.status, s.last.size.bytes, max_bytes[i]);
        const bool first = s.search.first;
        const uint32_t strength = s.search.next;
        pl_size_step(s.search, accepted);
        if (!accepted) {
            if (first) { s.kept = s.last; s.kept_in_stash = false; }     /* M does not fit: the image keeps the M result */
            continue;
        }
        /* the accepted probe with the smallest strength so far: every accepted probe lies below the one before it */
        s.kept = s.last; s.best = (long)strength; s.kept_in_stash = false;
        if (s.search.done) continue;                         /* (the chosen strength's result is in place) */
        stash.push_back(PlSearchMove{ i, PLA_IMAGE, PLA_BEST });
        stash.push_back(PlSearchMove{ i, PLA_FILTERS, PLA_BEST_FILTERS });
        if (want_streams) {
            stash.push_back(PlSearchMove{ i, PLA_ROWS, PLA_BEST_ROWS });
            stash.push_back(PlSearchMove{ i, PLA_IDS, PLA_BEST_IDS });
            s.kept_in_stash = true;
        }
    }
    return stash;
}

/* Close, target rule: the kept results back into the images whose last probe was refused (moved only with `commit`); `zero`: the images with no
 * accepted probe, which get strength 0 -- their originals back, then (with `commit`) ONE run of that group, after which pl_target_reran keeps
 * what it gave. */
struct PlTargetClose {
    std::vector<PlSearchMove> fin;
    std::vector<uint32_t> zero;
};
inline PlTargetClose pl_target_close(std::vector<PlTargetTrack> &st, bool commit)
{
    PlTargetClose c;
    for (size_t i = 0; i < st.size(); i++) {
        PlTargetTrack &s = st[i];
        if (s.search.failed) continue;
        if (s.in_place == (long)s.search.chosen) {
            if (s.best != (long)s.search.chosen) s.kept = s.last;        /* (M = 0 refused: the probe at 0 is what strength 0 gives) */
            continue;
        }
        if (s.best == (long)s.search.chosen) {
            if (commit) {
                c.fin.push_back(PlSearchMove{ (uint32_t)i, PLA_BEST, PLA_IMAGE });
                c.fin.push_back(PlSearchMove{ (uint32_t)i, PLA_BEST_FILTERS, PLA_FILTERS });
            }
            continue;
        }
        c.zero.push_back((uint32_t)i);
        s.kept = PlTargetProbe{};
        if (commit) c.fin.push_back(PlSearchMove{ (uint32_t)i, PLA_ORIG, PLA_IMAGE });
    }
    return c;
}
inline void pl_target_reran(std::vector<PlTargetTrack> &st, const std::vector<uint32_t> &zero)
{
    for (uint32_t i : zero) st[i].kept = st[i].last;
}

/* Close, size rule: the same moves.  The rule ends on an accepted probe, so what is not in place is in the stash; an image that was never probed
 * (one without pixels) has nothing to move. */
inline std::vector<PlSearchMove> pl_size_close(const std::vector<PlSizeTrack> &st, bool commit)
{
    std::vector<PlSearchMove> fin;
    for (size_t i = 0; i < st.size(); i++) {
        const PlSizeTrack &s = st[i];
        if (s.search.failed || s.in_place < 0 || s.in_place == (long)s.search.chosen || !commit) continue;
        fin.push_back(PlSearchMove{ (uint32_t)i, PLA_BEST, PLA_IMAGE });
        fin.push_back(PlSearchMove{ (uint32_t)i, PLA_BEST_FILTERS, PLA_FILTERS });
    }
    return fin;
}

#endif

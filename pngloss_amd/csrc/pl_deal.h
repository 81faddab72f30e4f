/*
 * pl_deal.h -- the index bookkeeping of the calls that take a batch of host images apart and put it together again: which context of a node gets
 * which image (pngloss_hip_multi_*), which images of a searched batch run together at their chosen strength (the host forms of the searches), and
 * what a call returns when its parts returned different codes.  Internal.
 *
 * Plain C++ without HIP, like pl_plan.h: pl_host_window.hip carries these out (threads, gathers, scatters), and tests/c/deal_host.cpp compiles the same
 * header with g++ so that the CPU suite pins them (tests/test_deal_host.py).
 */
#ifndef PL_DEAL_H
#define PL_DEAL_H

#include "../../include/pngloss_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

/* owner[i] = the part image i goes to.  LPT greedy, deterministic: images by descending pixel count (ties: lower index first), each to the least
 * loaded part (ties: lower part) -- the same rule as pngloss_amd/shard.py:lpt_partition.  parts < 1 counts as 1. */
inline std::vector<int> pl_deal_owners(const std::vector<uint64_t> &pixels, int parts)
{
    if (parts < 1) parts = 1;
    const size_t n = pixels.size();
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pixels[a] > pixels[b]; });
    std::vector<uint64_t> load((size_t)parts, 0);
    std::vector<int> owner(n, 0);
    for (size_t i : order) {
        int best = 0;
        for (int p = 1; p < parts; p++) if (load[(size_t)p] < load[(size_t)best]) best = p;
        owner[i] = best;
        load[(size_t)best] += pixels[i];
    }
    return owner;
}

/* The deal that owner[0 .. n) describes: part[p] = the images of part p, ascending; where[i] = (the part of image i, its index in part[that part]). */
struct PlDeal {
    std::vector<std::vector<size_t>> part;
    std::vector<std::pair<int, size_t>> where;
};
inline PlDeal pl_deal(const int *owner, size_t n, int parts)
{
    PlDeal d;
    d.part.resize((size_t)(parts < 1 ? 1 : parts));
    d.where.resize(n);
    for (size_t i = 0; i < n; i++) {
        std::vector<size_t> &mine = d.part[(size_t)owner[i]];
        d.where[i] = std::make_pair(owner[i], mine.size());
        mine.push_back(i);
    }
    return d;
}

/* The images of a batch by the strength each of them chose: one group per strength that occurs, strengths ascending, images ascending.  Each group
 * runs as one ordinary batch. */
inline std::vector<std::pair<uint32_t, std::vector<size_t>>> pl_strength_groups(const std::vector<uint32_t> &strength)
{
    std::vector<size_t> order(strength.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return strength[a] < strength[b]; });
    std::vector<std::pair<uint32_t, std::vector<size_t>>> out;
    for (size_t i : order) {
        if (out.empty() || out.back().first != strength[i]) out.emplace_back(strength[i], std::vector<size_t>());
        out.back().second.push_back(i);
    }
    return out;
}

/* The code of a call whose parts (chunks, contexts, strengths) returned codes of their own.  A hard error is anything but PNGLOSS_SUCCESS and
 * PNGLOSS_INTERNAL_ABORT (single images failed; they say so in their status, the others are good): the first hard error wins, else
 * PNGLOSS_INTERNAL_ABORT if any part returned it, else PNGLOSS_SUCCESS. */
inline bool pl_rc_is_hard(int rc) { return rc != PNGLOSS_SUCCESS && rc != PNGLOSS_INTERNAL_ABORT; }
inline int pl_fold_rc(int so_far, int rc) { return (pl_rc_is_hard(so_far) || rc == PNGLOSS_SUCCESS) ? so_far : rc; }
inline int pl_fold_rc(const std::vector<int> &rcs)
{
    int worst = PNGLOSS_SUCCESS;
    for (int rc : rcs) worst = pl_fold_rc(worst, rc);
    return worst;
}

#endif

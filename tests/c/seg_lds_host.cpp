/*
 * seg_lds_host.cpp -- TEST INFRASTRUCTURE: the shared-memory layouts of the segment engine's kernel bodies (pngloss_amd/csrc/pl_seg_lds.h, the header the bodies
 * take their pointers from and the launches their LDS bytes) behind a thin C ABI, so that the CPU suite proves alignment, order and overlays and pins every
 * launch's byte count without a GPU (tests/test_seg_lds_host.py).  One entry per instantiation the library ships.
 *
 *   seg_lds_host_layouts() -> number of layouts
 *   seg_lds_host_layout(k, n, name[64], out[2]) -> 0       out: regions, end in bytes (n: chain positions of the row; only the chain's layouts look at it)
 *   seg_lds_host_region(k, r, n, name[64], when[128], out[7]) -> 0   out: offset, element bytes, count, kind (0 own, 1 overlay, 2 overlay behind the row before),
 *                                                                         first, last (the rows an overlay of kind 1 lives in the place of; -1), alignment
 *   seg_lds_host_kernels() -> SEG_KERNEL_COUNT       seg_lds_host_kernel_name(kernel) -> its name
 *   seg_lds_host_launch_bytes(kernel, n) -> the LDS bytes of a launch of that kernel (n: the chain positions of the launch's widest row)
 *   seg_lds_host_constants(out[4]): SEG_UNIT, SEG_CHAIN_CAP8, SEG_CHAIN_CAP, SEG_UNT
 */
#include "../../pngloss_amd/csrc/pl_seg_launch.h"

#include <stdio.h>

namespace {

struct Entry { const char *name; int regions; SegLdsRegion (*region)(int, uint32_t); uint32_t (*end)(uint32_t); };
template <class L> Entry entry(const char *name)
{
    return Entry{ name, L::Table::n_regions, [](int i, uint32_t n) { return L::Table::region(i, n); }, [](uint32_t n) { return L::Table::end(n); } };
}

const Entry ENTRIES[] = {
    entry<SegLdsEnum<512>>("enum<512>"), entry<SegLdsEnum<1024>>("enum<1024>"),
    entry<SegLdsSeeded<512>>("seeded<512>"), entry<SegLdsSeeded<1024>>("seeded<1024>"),
    entry<SegLdsSmall<512>>("small<512>"), entry<SegLdsSmall<1024>>("small<1024>"),
    entry<SegLdsUnit<SEG_NSP, SEG_UNIT, SEG_UNC, false>>("unit_all<UNIT>"), entry<SegLdsUnit<SEG_SEED_LANES, SEG_UNIT, SEG_UNC_SEEDS_OF(SEG_UNIT), true>>("unit_seeds<UNIT>"),
    entry<SegLdsUnit<SEG_NSS, SEG_UNIT, SEG_UNC_SMALL_OF(SEG_UNIT), false>>("unit_small<UNIT>"),
    entry<SegLdsUnit<SEG_NSP, 1, SEG_UNC, false>>("unit_all<1>"), entry<SegLdsUnit<SEG_SEED_LANES, 1, SEG_UNC_SEEDS_OF(1), true>>("unit_seeds<1>"),
    entry<SegLdsUnit<SEG_NSS, 1, SEG_UNC_SMALL_OF(1), false>>("unit_small<1>"),
    entry<SegLdsFirst<512, false>>("first<512,false>"), entry<SegLdsFirst<1024, false>>("first<1024,false>"),
    entry<SegLdsFirst<SEG_UNT, true>>("first<UNT,true>"), entry<SegLdsFirst<SEG_UNT, false>>("first<UNT,false>"),
    entry<SegLdsChain<false>>("chain"), entry<SegLdsChain<true>>("chain_seeded"), entry<SegLdsChain<false>>("chain_unit"),
    entry<SegLdsExtremes>("extremes"),
    entry<SegLdsReplay>("replay<NT>"), entry<SegLdsReplay>("replay<NT_BATCH>"),
    entry<SegLdsPost<8>>("post<8>"), entry<SegLdsPost<16>>("post<16>"),
    entry<SegLdsCommit>("commit"),
    entry<SegLdsCtl>("ctl<TPARTS>"), entry<SegLdsCtl>("ctl<TPARTS_BATCH>"),
};
const int NENTRIES = (int)(sizeof(ENTRIES) / sizeof(ENTRIES[0]));

const char *const KERNELS[SEG_KERNEL_COUNT] = { "CTL", "CTL_BATCH", "ENUM_512", "ENUM_1024", "ENUM_SEEDED_512", "ENUM_SEEDED_1024", "ENUM_UNIT", "ENUM_UNIT1", "GATHER_SEEDED",
                                                "CHAIN", "CHAIN_SEEDED", "CHAIN_UNIT", "REPLAY", "REPLAY_BATCH" };

} // namespace

extern "C" {

int seg_lds_host_layouts(void) { return NENTRIES; }

int seg_lds_host_layout(int k, int64_t n, char *name, int64_t *out)
{
    if (k < 0 || k >= NENTRIES) return -1;
    snprintf(name, 64, "%s", ENTRIES[k].name);
    out[0] = ENTRIES[k].regions; out[1] = (int64_t)ENTRIES[k].end((uint32_t)n);
    return 0;
}

int seg_lds_host_region(int k, int r, int64_t n, char *name, char *when, int64_t *out)
{
    if (k < 0 || k >= NENTRIES || r < 0 || r >= ENTRIES[k].regions) return -1;
    const SegLdsRegion g = ENTRIES[k].region(r, (uint32_t)n);
    snprintf(name, 64, "%s", g.name);
    snprintf(when, 128, "%s", g.when ? g.when : "");
    out[0] = g.offset; out[1] = g.elem_bytes; out[2] = g.count; out[3] = g.kind; out[4] = g.first; out[5] = g.last; out[6] = g.align;
    return 0;
}

int seg_lds_host_kernels(void) { return SEG_KERNEL_COUNT; }
const char *seg_lds_host_kernel_name(int kernel) { return kernel >= 0 && kernel < SEG_KERNEL_COUNT ? KERNELS[kernel] : ""; }

/* through seg_attempt_launches: the byte count the launcher really hands to the kernel (a shape that makes the attempt launch that kernel; for the chain,
 * n positions: rows of n segments, or of n units) */
int64_t seg_lds_host_launch_bytes(int kernel, int64_t n)
{
    SegShape s = {};
    s.max_nseg = (uint32_t)(n > 0 ? n : 1); s.max_ngrp = 1; s.max_ncommit = 1; s.enum_nt = 512; s.tparts = SEG_TPARTS; s.unit = 1; s.small_ok = true;
    switch ((SegKernel)kernel) {
    case SEG_KERNEL_CTL: case SEG_KERNEL_ENUM_512: case SEG_KERNEL_CHAIN: case SEG_KERNEL_REPLAY: break;
    case SEG_KERNEL_CTL_BATCH: case SEG_KERNEL_ENUM_UNIT: case SEG_KERNEL_CHAIN_UNIT: case SEG_KERNEL_REPLAY_BATCH:
        s.tparts = SEG_TPARTS_BATCH; s.unit = SEG_UNIT; s.max_nseg = (uint32_t)(n > 0 ? n : 1) * SEG_UNIT; break;
    case SEG_KERNEL_ENUM_1024: s.enum_nt = 1024; break;
    case SEG_KERNEL_ENUM_SEEDED_512: case SEG_KERNEL_CHAIN_SEEDED: case SEG_KERNEL_GATHER_SEEDED: s.seeded = true; s.max_nseg = s.max_nseg < 2 && kernel == SEG_KERNEL_GATHER_SEEDED ? 2 : s.max_nseg; break;
    case SEG_KERNEL_ENUM_SEEDED_1024: s.seeded = true; s.enum_nt = 1024; break;
    case SEG_KERNEL_ENUM_UNIT1: s.seeds = true; break;
    case SEG_KERNEL_COUNT: return -1;
    }
    SegLaunch L[SEG_MAX_LAUNCHES];
    const int nl = seg_attempt_launches(s, L);
    for (int i = 0; i < nl; i++) if (L[i].kernel == (SegKernel)kernel) return (int64_t)L[i].lds_bytes;
    return -1;
}

void seg_lds_host_constants(int64_t *out) { out[0] = SEG_UNIT; out[1] = SEG_CHAIN_CAP8; out[2] = SEG_CHAIN_CAP; out[3] = SEG_UNT; }

} /* extern "C" */

/*
 * wg_lds_host.cpp -- TEST INFRASTRUCTURE: the shared memory of the workgroup engine (pngloss_amd/csrc/pl_wg_lds.h, the header pl_engine.hip takes its offsets and
 * its launch's LDS bytes from) behind a thin C ABI, so that the CPU suite proves alignment, order and fit and pins every byte count without a GPU
 * (tests/test_wg_lds_host.py).
 *
 *   wg_lds_host_place(region, grow_bytes, align, head[6]) -> number of entries (one per slot of every region), or -1
 *        places the header's table -- or, region >= 0, a COPY of it with that region's slots grown by grow_bytes and (align > 0) its alignment replaced --
 *        with the header's own pl_wg_place.  head: sound (what the header's static_assert looks at), union offset, union bytes, launch bytes, regions,
 *        pixels the commit view holds
 *   wg_lds_host_entry(i, name[64], out[6]) -> 0      of the last placement.  out: view, region, slot, offset, bytes, alignment
 *   wg_lds_host_constants(out[12])                    the sizes the layout is made of
 *   wg_lds_host_chain_slot(what, i)                   0: first round-1 slot of wave i, 1: how many it takes, 2: decision table of filter i, 3: record slots of filter i
 *   wg_lds_host_named(out[24])                        the named slots: the seven flag words (in the kernel's order of declaration), work, pacc, phase clocks
 */
#include "../../pngloss_amd/csrc/pl_wg_lds.h"

#include <stdio.h>

namespace {

struct Entry { const char *name; int view, region, slot; uint32_t offset, bytes, align; };
Entry g_entries[64];
int g_n = 0;

} // namespace

extern "C" {

int wg_lds_host_place(int region, int grow_bytes, int align, int64_t *head)
{
    PlWgRegion t[PL_WG_REGIONS];
    for (int k = 0; k < PL_WG_REGIONS; k++) t[k] = PL_WG_TABLE[k];
    if (region >= PL_WG_REGIONS) return -1;
    if (region >= 0) {
        if (grow_bytes % (int)t[region].elem_bytes || t[region].count == PL_WG_FILL) return -1;
        t[region].count += (uint32_t)(grow_bytes / (int)t[region].elem_bytes);
        if (align > 0) t[region].align = (uint32_t)align;
    }
    const PlWgPlaced p = pl_wg_place(t, PL_WG_REGIONS);
    g_n = 0;
    for (int k = 0; k < PL_WG_REGIONS; k++)
        for (uint32_t s = 0; s < t[k].slots && g_n < 64; s++) {
            const uint32_t b = pl_wg_slot_bytes(t[k], p.count[k]);
            g_entries[g_n++] = Entry{ t[k].name, t[k].view, k, (int)s, p.off[k] + s * b, b, t[k].align };
        }
    head[0] = p.sound; head[1] = p.union_off; head[2] = p.union_bytes; head[3] = p.launch_bytes; head[4] = PL_WG_REGIONS;
    head[5] = p.count[PL_WG_R_TTERMS];
    return g_n;
}

int wg_lds_host_entry(int i, char *name, int64_t *out)
{
    if (i < 0 || i >= g_n) return -1;
    const Entry &e = g_entries[i];
    snprintf(name, 64, "%s", e.name);
    out[0] = e.view; out[1] = e.region; out[2] = e.slot; out[3] = e.offset; out[4] = e.bytes; out[5] = e.align;
    return 0;
}

void wg_lds_host_constants(int64_t *out)
{
    out[0] = PL_NFILT; out[1] = PL_NSYM; out[2] = PL_TBL_N; out[3] = PL_TBL_DUMMY; out[4] = PL_CHUNK; out[5] = PL_LT_N; out[6] = PL_LCHUNK;
    out[7] = PL_LREC_N; out[8] = PL_LRING_N; out[9] = PL_LREC_BYTES; out[10] = PL_LOUT_BYTES; out[11] = PL_WG_ALIGN_SLACK;
}

int wg_lds_host_chain_slot(int what, int i)
{
    switch (what) {
    case 0: return pl_wg_round1_slot(i);
    case 1: return pl_wg_round1_slots(i);
    case 2: return pl_wg_lead_table(i);
    case 3: return pl_wg_lead_rec_slots(i);
    default: return -1;
    }
}

void wg_lds_host_named(int64_t *out)
{
    const int64_t v[24] = { PL_WG_F_BIG_ERR, PL_WG_F_BIG_LEAD, PL_WG_F_UNIQ, PL_WG_F_SIMD_MAP, PL_WG_F_CHAINS_DONE, PL_WG_F_POST_DONE, PL_WG_F_ROWCYC,
                            PL_LW_RESCAN, PL_LW_BUMPED, PL_LW_NREL, PL_LW_MARKX, PL_LW_REL, PL_LREL_MAX, PL_LW_CLOSE, PL_LWORK_N,
                            PL_PA_DERR, PL_PA_COST, PL_PA_HS, PL_PA_WORDS,
                            PL_CC_N, PL_LC_N, PL_LC_BUILD, PL_CC_FLUSH, PL_LC_FLUSH };
    for (int i = 0; i < 24; i++) out[i] = v[i];
}

} /* extern "C" */

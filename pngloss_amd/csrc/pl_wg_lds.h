/*
 * pl_wg_lds.h -- the SHARED MEMORY (LDS) of the workgroup engine (pl_engine.hip: one workgroup per image), stated once: one table of regions in carve
 * order -- a fixed part, and behind it a union that three phases of a row look at in three ways (the round-1 chains, the band-leader chains, the commit
 * pass) -- from which every offset the kernel uses and the bytes its launch asks for come as compile-time constants.  Also the named slots of the small
 * bookkeeping arrays (flag words, a chain's work array, the post pass accumulators, the chains' phase clocks).  Internal.
 *
 * Plain C++17, no HIP: the kernel compiles it, and so does tests/c/wg_lds_host.cpp, which lists every region for tests/test_wg_lds_host.py (alignment, order,
 * no overlap, every view inside the union, every chain's needs inside its slot, every byte count pinned).  A region that misses its alignment or a view that
 * leaves the union does not compile.
 */
#ifndef PL_WG_LDS_H
#define PL_WG_LDS_H

#include <stdint.h>
#include <type_traits>

/* (pl_device.h's, stated again token for token for a compile without HIP: a redefinition that differs is diagnosed) */
#define PL_NFILT 5
#define PL_NSYM 256

/* ---- sizes the layout is made of (the chains use them too) ------------------------------------------------------------------------------------------------ */
/* (PL_TBL_N and PL_LWORK_N can be set from the command line: the tests compile the layout with a wrong size and expect the asserts below to refuse it) */
#define PL_TBL_DUMMY 64             /* slots behind the bins of a histogram table, one per lane: a lane that bumps nothing adds 0 to its own (chain_row) */
#ifndef PL_TBL_N
#define PL_TBL_N 512                /* entries of a histogram table: 256 bins + the dummy slots, padded so that every table is 4 KB and 4 KB aligned */
#endif
#define PL_TBL_ALIGN 4096           /* the band-leader chain ORs the bin offset into the table address */
#define PL_CHUNK 32                 /* round-1 chains: pixels per vector pre-phase; small so that several workgroups fit one CU's LDS */
#define PL_LT_N 512                 /* decision-table entries per chain: filt in [-256, 255] */
#define PL_LCHUNK 64                /* band-leader chains: pixels per vector phase */
#ifndef PL_LWORK_N
#define PL_LWORK_N 128              /* words of a chain's work array (slots: PL_LW_*) */
#endif
#define PL_LREL_MAX 64              /* watched relations a chain can list */
#define PL_LREC_OVER 8              /* records behind the chunk's: the hand-scheduled loop runs whole groups of four, up to 4 pixels past the chunk, and fetches 2
                                       ahead (6), and eight lanes write the neutral records */
#define PL_LREC_N (PL_LCHUNK + PL_LREC_OVER)
#define PL_LRING_N (2 + PL_LCHUNK + PL_LREC_OVER)   /* pixels of a result ring: the two in front of the chunk, the chunk, and what the overshooting loop writes behind it */
/* the strides the generated loops (pl_lead_asm.h, tools/gen_lead_asm.py) have in their offsets: */
#define PL_LREC_BYTES 16            /* a chain record: one ds_read_b128; 4 channels a pixel, (paeth: two records a channel) = 64 or 128 bytes a pixel */
#define PL_LOUT_BYTES 8             /* a result: one ds_write_b64; 4 channels = 32 bytes a pixel */
#define PL_WG_ALIGN_SLACK 4096      /* the launch asks for this much more: the kernel rounds the dynamic LDS's base up to PL_TBL_ALIGN */

/* ---- named slots ------------------------------------------------------------------------------------------------------------------------------------------ */
/* the flag words (region flags, one word each) */
enum { PL_WG_F_BIG_ERR = 0,         /* some |incoming error| of the coming row exceeds 8000 (see WRAP) */
       PL_WG_F_BIG_LEAD = 1,        /* ... exceeds PL_E0_LEAD_MAX: the row takes the round-1 chain */
       PL_WG_F_UNIQ = 2,            /* epilogue: distinct symbols */
       PL_WG_F_SIMD_MAP = 3,        /* diagnostics */
       PL_WG_F_ROWCYC = 4,          /* cycles of the slowest chain wave of this row attempt */
       PL_WG_F_CHAINS_DONE = 5,     /* chain waves that finished this row attempt */
       PL_WG_F_POST_DONE = 6,       /* candidates whose post pass their own wave already did */
       PL_WG_F_USED = 7, PL_WG_F_WORDS = 16 };
/* a band-leader chain's work array (LeadCtx::work, PL_LWORK_N words) */
enum { PL_LW_RESCAN = 0,            /* [8] ids of the bands lead_rescan rescanned (-1: none), slot 2 * channel + sign */
       PL_LW_BUMPED = 32,           /* [8] flush_verify: bitmap of the bins the range bumps */
       PL_LW_NREL = 41,             /* number of watched relations */
       PL_LW_MARKX = 42,            /* the pixel the row stood at when the close relations were marked */
       PL_LW_REL = 48,              /* [PL_LREL_MAX] the relations: leader bin u | bin l of the other band's leader << 8 */
       PL_LW_CLOSE = 112,           /* [8] bitmap of the bins u of the relations that were close then */
       PL_LW_USED = 120 };
/* the post pass accumulators (region pacc): PL_PA_WORDS per candidate */
enum { PL_PA_DERR = 0,              /* derivative error, 64 bit: low word, high word (one 64-bit atomic add) */
       PL_PA_COST = 2,              /* entropy cost */
       PL_PA_HS = 3,                /* + g: libpng's heuristic sum of filter g */
       PL_PA_WORDS = 8 };
/* phase clocks of a band-leader chain (LeadCtx::cyc) ... */
enum { PL_CC_VEC = 0, PL_CC_FAST = 1, PL_CC_EXACT = 2, PL_CC_RESCAN = 3,
       PL_CC_CLEAN = 4,             /* cycles of undisturbed whole-chunk runs ... */
       PL_CC_CLEAN_PX = 5,          /* ... and their pixels */
       PL_CC_FLUSH = 6,             /* flush + relation check */
       PL_CC_N = 7 };
/* ... and what the kernel sums them into, over the rows (lead_cyc; the first PLR_WG_PHASES go out as PLR_WG_PHASE_KCYC) */
enum { PL_LC_VEC = 0, PL_LC_FAST = 1, PL_LC_EXACT = 2, PL_LC_RESCAN = 3,
       PL_LC_BUILD = 4,             /* table build (measured by the kernel around lead_build_table) */
       PL_LC_CLEAN = 5, PL_LC_CLEAN_PX = 6, PL_LC_FLUSH = 7,
       PL_LC_N = 8 };
static_assert((int)PL_CC_VEC == (int)PL_LC_VEC && (int)PL_CC_FAST == (int)PL_LC_FAST && (int)PL_CC_EXACT == (int)PL_LC_EXACT && (int)PL_CC_RESCAN == (int)PL_LC_RESCAN,
              "the kernel adds the first four phases of a chain by position");
static_assert(PL_WG_F_USED <= PL_WG_F_WORDS && PL_LW_USED <= PL_LWORK_N && PL_LW_REL + PL_LREL_MAX <= PL_LW_CLOSE && PL_PA_HS + PL_NFILT <= PL_PA_WORDS,
              "named slots inside their arrays");

/* ---- the table -------------------------------------------------------------------------------------------------------------------------------------------- */
enum { PL_WG_FIXED = 0,             /* lives for the whole kernel */
       PL_WG_ROUND1 = 1,            /* the union while the round-1 chains run a row (chain_row) */
       PL_WG_LEAD = 2,              /* ... while the band-leader chains do (chain_lead) */
       PL_WG_COMMIT = 3,            /* ... in the commit pass, when no chain runs */
       PL_WG_VIEWS = 4 };
#define PL_WG_FILL 0xFFFFFFFFu      /* a count: as many elements as the union holds */
/* `slots` equal arrays of `count` elements one behind the other (one per candidate filter, mostly); the first starts on a multiple of `align`, and where
 * there are several their size is a multiple of it, too */
struct PlWgRegion { const char *name; int view; uint32_t elem_bytes, count, slots, align; };
enum { PL_WG_R_TBL, PL_WG_R_HC, PL_WG_R_SPLIT_LUT, PL_WG_R_SPLIT_LUT2, PL_WG_R_COSTS, PL_WG_R_PACC, PL_WG_R_FLAGS,
       PL_WG_R_REC,
       PL_WG_R_LTAB, PL_WG_R_LBS, PL_WG_R_LWORK, PL_WG_R_LREC, PL_WG_R_LOUT,
       PL_WG_R_TTERMS,
       PL_WG_REGIONS };
constexpr PlWgRegion PL_WG_TABLE[PL_WG_REGIONS] = {
    /* {running symbol_frequency, rank(original_frequency) << 9} per candidate filter (+ the dummy slots) */
    { "tbl", PL_WG_FIXED, 8, PL_TBL_N, PL_NFILT, PL_TBL_ALIGN },
    { "Hc", PL_WG_FIXED, 4, PL_NSYM, 1, 4 },                    /* committed symbol_frequency */
    { "split_lut", PL_WG_FIXED, 4, 512, 1, 4 },                 /* [diff+256] -> rem | thr<<16 of the Sierra split, |diff| <= 255 */
    { "split_lut2", PL_WG_FIXED, 4, 512, 1, 4 },                /* [diff+256] -> twos | fours << 8 | five << 16 | threes << 24 (int8 each): the next-rows terms, for the commit pass */
    { "costs", PL_WG_FIXED, 8, 8, 1, 8 },                       /* the candidates' row costs (five used) */
    { "pacc", PL_WG_FIXED, 4, PL_PA_WORDS, PL_NFILT, 8 },       /* post pass accumulators (PL_PA_*); 8: the 64-bit atomic add into PL_PA_DERR */
    { "flags", PL_WG_FIXED, 4, PL_WG_F_WORDS, 1, 4 },           /* PL_WG_F_* */
    /* round-1 chains: chunk records [PL_CHUNK][4][1 or 2] of 16 bytes.  Wave 0 (two filters side by side: two records a channel) takes slots 0 and 1, waves
     * 1..4 slots 2..5 (pl_wg_round1_slot) */
    { "rec", PL_WG_ROUND1, 16, PL_CHUNK * 4, 6, 16 },
    /* band-leader chains: six decision tables (filter none has two: P pixels, and PL_LT_N * 8 bytes behind it N pixels; then sub, up, average, paeth:
     * pl_wg_lead_table) */
    { "ltab", PL_WG_LEAD, 8, PL_LT_N, PL_NFILT + 1, 8 },
    { "lbs", PL_WG_LEAD, 4, 512, PL_NFILT, 4 },                 /* band states */
    { "lwork", PL_WG_LEAD, 4, PL_LWORK_N, PL_NFILT, 4 },        /* PL_LW_* */
    { "lrec", PL_WG_LEAD, PL_LREC_BYTES, PL_LREC_N * 4, PL_NFILT + 1, 16 },   /* chain records [PL_LREC_N][4]; none, sub, up, average, and paeth, whose two records a channel take the last two slots */
    { "lout", PL_WG_LEAD, PL_LOUT_BYTES, PL_LRING_N * 4, PL_NFILT, 8 },       /* result rings [PL_LRING_N][4] */
    /* commit pass: the next-rows terms of every pixel of the row, four words, where the row fits; wider rows take the pass that needs no LDS */
    { "tterms", PL_WG_COMMIT, 16, PL_WG_FILL, 1, 16 },
};

struct PlWgPlaced {
    uint32_t off[PL_WG_REGIONS], count[PL_WG_REGIONS];   /* count: elements of a slot (a PL_WG_FILL resolved) */
    uint32_t union_off, union_bytes;                     /* the union starts where the fixed part ends and is as large as its largest chain view */
    uint32_t view_end[PL_WG_VIEWS];
    uint32_t launch_bytes;
    bool sound;
};
constexpr uint32_t pl_wg_slot_bytes(const PlWgRegion &r, uint32_t count) { return r.elem_bytes * count; }
constexpr PlWgPlaced pl_wg_place(const PlWgRegion *t, int n)
{
    PlWgPlaced p = {};
    p.sound = n == PL_WG_REGIONS;
    for (int pass = 0; pass < 3; pass++) {          /* the fixed part; the chain views, which size the union; the commit view, which fills it */
        for (int v = 0; v < PL_WG_VIEWS; v++) {
            if ((pass == 0) != (v == PL_WG_FIXED) || (pass == 2) != (v == PL_WG_COMMIT)) continue;
            uint32_t at = v == PL_WG_FIXED ? 0u : p.union_off;
            for (int k = 0; k < n; k++) {
                if (t[k].view != v) continue;
                p.off[k] = at;
                p.count[k] = t[k].count == PL_WG_FILL ? (p.union_off + p.union_bytes - at) / t[k].elem_bytes : t[k].count;
                at += pl_wg_slot_bytes(t[k], p.count[k]) * t[k].slots;
            }
            p.view_end[v] = at;
            if (v == PL_WG_FIXED) p.union_off = at;
            else if (pass == 1 && at - p.union_off > p.union_bytes) p.union_bytes = at - p.union_off;
        }
    }
    p.launch_bytes = PL_WG_ALIGN_SLACK + p.union_off + p.union_bytes;
    for (int k = 0; k < n; k++) {
        if (k && t[k].view < t[k - 1].view) p.sound = false;                                          /* carve order: view by view */
        if (!t[k].elem_bytes || !p.count[k] || !t[k].slots || !t[k].align) { p.sound = false; continue; }
        if (p.off[k] % t[k].align) p.sound = false;
        if (t[k].slots > 1 && pl_wg_slot_bytes(t[k], p.count[k]) % t[k].align) p.sound = false;
    }
    for (int v = 1; v < PL_WG_VIEWS; v++) if (p.view_end[v] > p.union_off + p.union_bytes) p.sound = false;
    return p;
}
constexpr PlWgPlaced PL_WG_LDS = pl_wg_place(PL_WG_TABLE, PL_WG_REGIONS);
static_assert(PL_WG_LDS.sound, "pl_wg_lds.h: a region misses its alignment or a view leaves the union");

/* compile-time values (never a read of PL_WG_LDS at run time): byte offset of a region from the aligned base, bytes of one of its slots */
#define PL_WG_OFF(r) (std::integral_constant<uint32_t, PL_WG_LDS.off[PL_WG_R_##r]>::value)
#define PL_WG_SLOT(r) (std::integral_constant<uint32_t, pl_wg_slot_bytes(PL_WG_TABLE[PL_WG_R_##r], PL_WG_LDS.count[PL_WG_R_##r])>::value)
#define PL_WG_UNION_BYTES (std::integral_constant<uint32_t, PL_WG_LDS.union_bytes>::value)      /* what the commit pass may use of the chains' region */
#define PL_WG_LAUNCH_BYTES (std::integral_constant<uint32_t, PL_WG_LDS.launch_bytes>::value)

/* ---- which slot a chain takes, and that what it does there stays inside ----------------------------------------------------------------------------------- */
constexpr int pl_wg_round1_slot(int wave) { return wave == 0 ? 0 : 1 + wave; }                 /* wave 0 has two */
constexpr int pl_wg_round1_slots(int wave) { return wave == 0 ? 2 : 1; }
constexpr int pl_wg_lead_table(int f) { return f ? f + 1 : 0; }                                /* filter none has two */
constexpr int pl_wg_lead_rec_slots(int f) { return f == PL_NFILT - 1 ? 2 : 1; }                /* paeth has two (records: slot f) */
static_assert(PL_WG_SLOT(TBL) == PL_TBL_ALIGN && (PL_NSYM + PL_TBL_DUMMY) * 8 <= PL_WG_SLOT(TBL), "a histogram table is its bins and dummy slots in exactly 4 KB");
static_assert(PL_WG_SLOT(LTAB) == PL_LT_N * 8, "chain_lead hops PL_LT_N * 8 bytes from filter none's first decision table to its second");
static_assert(pl_wg_round1_slot(PL_NFILT - 1) + pl_wg_round1_slots(PL_NFILT - 1) <= (int)PL_WG_TABLE[PL_WG_R_REC].slots
              && PL_CHUNK * 4 * 2 * 16 <= pl_wg_round1_slots(0) * PL_WG_SLOT(REC), "round-1 records: every wave's slots exist, wave 0's pairs fit its two");
static_assert(pl_wg_lead_table(PL_NFILT - 1) < (int)PL_WG_TABLE[PL_WG_R_LTAB].slots && pl_wg_lead_table(1) == 2, "decision tables: one for every chain, two for none");
static_assert(PL_NFILT - 1 + pl_wg_lead_rec_slots(PL_NFILT - 1) <= (int)PL_WG_TABLE[PL_WG_R_LREC].slots
              && (PL_LCHUNK + 4 + 2) * 4 * PL_LREC_BYTES <= PL_WG_SLOT(LREC), "chain records: the overshooting loop stays inside a slot, paeth inside its two");
static_assert((PL_LCHUNK * 4 + 7) * PL_LOUT_BYTES < PL_WG_SLOT(LOUT) && (2 + PL_LCHUNK + 4) * 4 * PL_LOUT_BYTES <= PL_WG_SLOT(LOUT),
              "result ring: the last two results are read at [n * 4 + 0..7], the overshooting loop writes up to 4 pixels behind the chunk");

#endif

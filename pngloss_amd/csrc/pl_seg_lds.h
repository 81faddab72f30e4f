/*
 * pl_seg_lds.h -- the SHARED MEMORY (LDS) of the segment engine's kernel bodies, stated once: for every body one layout -- its regions in carve order,
 * each with a name, an element type and a count -- from which both come: the pointers the body works with (one typed accessor per region, its offset a
 * compile-time constant) and the bytes its launch asks for (the largest end among the bodies a kernel dispatches, plus a named pad).  Internal.
 *
 * Plain C++17 plus the macros and records of pl_seg_core.h, no HIP; pl_seg_core.h includes it between those and the kernel bodies (it is not a header to
 * include by itself).  The bodies take their pointers from here, pl_seg_launch.h and pl_seg.hip their byte counts, and tests/c/seg_lds_host.cpp lists every region of every shipped instantiation for tests/test_seg_lds_host.py (alignment,
 * no overlap, every overlay inside its host, every launch at least as large as every body it carries, every byte count pinned).
 *
 * A layout is an X-macro list of rows, in carve order:
 *   R(name, type, address space, count)                    a region of its own, behind the one before
 *   O(name, type, address space, count, first, last, when) an OVERLAY: lives in the place of regions first .. last (from first's start), valid `when`
 *   B(name, type, address space, count)                    ... and the next overlay of the same place, behind the row before
 *   V(name, type, address space, count)                    (the chain) a region behind one whose size depends on the row's chain positions n: its offset
 *                                                          is a function of n, the accessor takes n
 * Address space: SEG_AS_LDS where the body works with LDS pointers, nothing where it works with generic ones (what each body did before this table existed:
 * the generated code is the same).  A count of SEG_LDS_FITS says: as many bytes as the overlays placed there need.
 * A region starts on a multiple of its ALIGNMENT: its element size, or what the layout's ALIGN list states where a body accesses it with something wider.
 * An overlay that does not fit its place, or a region that does not start on a multiple of its alignment, does not compile (SEG_LDS_LAYOUT).
 */
#ifndef PL_SEG_LDS_H
#define PL_SEG_LDS_H

#ifndef PL_SEG_CORE_H
#error "pl_seg_lds.h is a part of pl_seg_core.h: include that"
#endif

/* ---- sizes the layouts are made of (the bodies use them too) ---------------------------------------------------------------------------------------------- */
#define SEG_HT 512                /* seg_enum_body: slots of a channel's hash table */
#ifndef SEG_UNC_SMALL
#define SEG_UNC_SMALL (SEG_UNIT <= 3 ? 20 : (SEG_UNIT <= 4 ? 15 : (SEG_UNIT <= 6 ? 10 : 7)))          /* (unit, channel) pairs per workgroup for none / up with their small state set */
#endif
#define SEG_UNC_SMALL_OF(unit) ((unit) == SEG_UNIT ? SEG_UNC_SMALL : (SEG_UNC_SMALL < 20 ? SEG_UNC_SMALL : 20))      /* ... and segment by segment (round 6: seg_k_enum_unit<1>) */
#define SEG_UNPX (SEG_UNC_SMALL * (SEG_UNIT * SEG_L + 1))   /* pixel records of a workgroup's pairs */
#define SEG_UN_K1MAX 4
#define SEG_CBLK 16
#define SEG_CR_SH 6
#define SEG_CR_MAX (1 << SEG_CR_SH)                             /* the usual table stride; the exit states are staged in shared memory at this stride */
#define SEG_CHAIN_CAP 256                                       /* most transitions of a pass (strides 64 and 128) */
#define SEG_CHAIN_CAP8 224                                      /* ... at stride 256 */
#define SEG_CHAIN_POS (SEG_CHAIN_CAP + 32)                      /* dn / entL entries */
#define SEG_CHAIN_TROWS(n) (((n) < SEG_CHAIN_CAP8 ? (n) : SEG_CHAIN_CAP8) + SEG_CBLK + 2)
#define SEG_CHAIN_TBYTES(n) ((size_t)SEG_CHAIN_TROWS(n) * 512)     /* T (and R behind it at the usual stride) for a row of n segments: the widest stride sets the size */
#define SEG_CHAIN_GWORDS ((SEG_CHAIN_CAP / SEG_CBLK + 2) * 256 / 2)
#ifndef SEG_WATCH_OF
#define SEG_WATCH_OF(V) ((V) > 8 ? 2 : 8)   /* slots of exact prefix counts a validation workgroup has for the bins its undecided decisions name (a bin without a slot is counted by scanning: exact, slower, rare -- 0.01 % of the decisions are undecided at all); two for whole replay groups: with 51 KB instead of 64 a CU takes a third enumeration workgroup next to such a workgroup */
#endif
#define SEG_BINB_STRIDE (SEG_L * 4 + 4)
#define SEG_PC_SEG (SEG_L + 1)                   /* words per segment and slot (one pad word: bank spread) */
#define SEG_PC_STRIDE_V(V) ((V) * SEG_PC_SEG + 8)
#define SEG_NBAND 20
#define SEG_CTLC_WORDS ((sizeof(SegCtl) + 7) / 8 * 2)          /* the control block and the sums, copied into shared memory: whole 64-bit words */
#define SEG_ACCC_WORDS ((sizeof(SegAcc) + 7) / 8 * 2)
#define SEG_DEC_WORDS 20                                      /* seg_decide_wg shares a SegDecision through this many words ... */
#define SEG_DEC_COST_WORD 6                                   /* ... and seg_ctl_body reads SegDecision::cost[f] out of the shared copy by word index (both asserted at SegDecision) */

/* ---- named slots of the small bookkeeping regions --------------------------------------------------------------------------------------------------------- */
/* trflag of seg_enum_body_k / seg_enum_seeded_body, [8] */
enum { SEG_TF_TRANSPARENT = 0,    /* some pixel of the segment (seeded: of the window) is fully transparent */
       SEG_TF_NDISTINCT = 1,      /* + channel: distinct states (seeded: distinct entry states) of the workgroup's channel */
       SEG_TF_WSIMD = 6,          /* (seg_enum_body_k, SEG_EXPERIMENT_TAIL_PLACEMENT only) the SIMD of every wave, two bits each */
       SEG_TF_HWID0 = 7,          /* (seg_enum_body_k, SEG_EXPERIMENT_TAIL_PLACEMENT only) HW_ID of wave 0 */
       SEG_TF_NRUNIN = 3 };       /* + channel (seeded, two stages, a channel pair per workgroup: the slots of the channels it does not have): distinct states after the run-in's first steps */
/* misc of seg_enum_unit_body, [128] */
enum { SEG_UM_TRANSPARENT = 0,    /* transparent pixel seen */
       SEG_UM_TURN_N = 8,         /* + kk: distinct states of the turn's pair kk */
       SEG_UM_POOL = 32,          /* + k: first pool slot of pair k (.. + NC = total) */
       SEG_UM_POOL2 = 64,         /* + k: the same for the SECOND list (.. + NC = its total) */
       SEG_UM_LANEBITS = 96 };    /* .. 127: one bit per lane: it represents a state of the second list */
/* idxb of seg_chain_body, [32] */
enum { SEG_CI_REPAIRS = 24,       /* segments walked step by step / rows broken off */
       SEG_CI_NOID = 25,          /* first position without an id */
       SEG_CI_ENTRY0 = 26,        /* entry state of the pass's first position */
       SEG_CI_DMAX = 27,          /* most distinct states of a segment */
       SEG_CI_START_ID = 28,      /* dense id the pass starts with */
       SEG_CI_WIDE = 30,          /* some segment has more distinct states than the stride */
       SEG_CI_TABLES = 31 };      /* repair tables loaded */
/* mm of seg_extremes_body, [2]: biased (unsigned compare) */
enum { SEG_MM_MAX = 0, SEG_MM_MIN = 1 };
/* red of seg_replay_body, [16] */
enum { SEG_RR_DERR = 0,           /* lo, hi */
       SEG_RR_HS = 2,             /* + g: hs[5] */
       SEG_RR_LB = 10,            /* lo, hi */
       SEG_RR_REACH = 12,
       SEG_RR_MAX = 14, SEG_RR_MIN = 15 };   /* biased: unsigned max / min */
/* red of seg_post_body, [64] (the first sixteen are initialised) */
enum { SEG_PR_FAIL = 8,           /* smallest failing decision index, or SEG_NOFAIL */
       SEG_PR_LEFT = 9,           /* the bytes of the pixel in front of the group */
       SEG_PR_PENDING = 13 };     /* (phase clocks) decisions that waited for the exact pass */
/* wbits of seg_post_body / SegVal, [32]: [0 .. 8) the bitmap of the watched bins */
enum { SEG_WB_PENDING = 8,        /* pending decisions, then: slots in use */
       SEG_WB_BIN = 9 };          /* + slot: the bin of each slot */

/* ---- the table machinery ---------------------------------------------------------------------------------------------------------------------------------- */
#define SEG_LDS_FITS 0xFFFFFFFFu
#define SEG_LDS_MAX_ROWS 24
/* a row as the list states it, then (seg_lds_place) with its offset: what a test enumerates */
struct SegLdsRegion {
    const char *name;
    uint32_t offset, elem_bytes, count;
    uint32_t align;                       /* it starts on a multiple of this: its element size, or what the layout's ALIGN list says (the widest access the body makes) */
    int kind;                             /* 0 R / V, 1 O, 2 B */
    int first, last;                      /* an overlay: the rows in whose place it lives; -1: a region of its own */
    const char *when;                     /* ... and when it is valid */
};
struct SegLdsPlaced { uint32_t off[SEG_LDS_MAX_ROWS], bytes[SEG_LDS_MAX_ROWS], end; bool sound; };
constexpr SegLdsPlaced seg_lds_place(const SegLdsRegion *t, int n)
{
    SegLdsPlaced p = {};
    uint32_t rel[SEG_LDS_MAX_ROWS] = {};
    int first[SEG_LDS_MAX_ROWS] = {}, last[SEG_LDS_MAX_ROWS] = {};
    for (int k = 0; k < n; k++) {                   /* an overlay's place, and its offset from that place's start */
        first[k] = t[k].kind == 2 ? first[k - 1] : t[k].first; last[k] = t[k].kind == 2 ? last[k - 1] : t[k].last;
        p.bytes[k] = t[k].count == SEG_LDS_FITS ? 0u : t[k].elem_bytes * t[k].count;
        rel[k] = t[k].kind == 2 ? rel[k - 1] + p.bytes[k - 1] : 0u;
    }
    for (int k = 0; k < n; k++)                     /* a place that is as large as its overlays need */
        if (t[k].count == SEG_LDS_FITS)
            for (int q = 0; q < n; q++) if (t[q].kind && first[q] == k && last[q] == k && rel[q] + p.bytes[q] > p.bytes[k]) p.bytes[k] = rel[q] + p.bytes[q];
    for (int k = 0; k < n; k++) if (!t[k].kind) { p.off[k] = p.end; p.end += p.bytes[k]; }
    p.sound = n <= SEG_LDS_MAX_ROWS;
    for (int k = 0; k < n; k++) {
        if (t[k].kind) { p.off[k] = p.off[first[k]] + rel[k]; if (p.off[k] + p.bytes[k] > p.off[last[k]] + p.bytes[last[k]]) p.sound = false; }
        if (p.off[k] % t[k].align) p.sound = false;
    }
    return p;
}
constexpr uint32_t seg_lds_max(uint32_t a) { return a; }
template <class... R> constexpr uint32_t seg_lds_max(uint32_t a, R... r) { return a > seg_lds_max(r...) ? a : seg_lds_max(r...); }

#define SEG_LDS_ID_R(name, T, AS, n) i_##name,
#define SEG_LDS_ID_O(name, T, AS, n, first, last, when) i_##name,
#define SEG_LDS_ROW_R(name, T, AS, n) SegLdsRegion{ #name, 0u, (uint32_t)sizeof(T), (uint32_t)(n), (uint32_t)sizeof(T), 0, -1, -1, nullptr },
#define SEG_LDS_ROW_O(name, T, AS, n, first, last, when) SegLdsRegion{ #name, 0u, (uint32_t)sizeof(T), (uint32_t)(n), (uint32_t)sizeof(T), 1, i_##first, i_##last, when },
#define SEG_LDS_ROW_B(name, T, AS, n) SegLdsRegion{ #name, 0u, (uint32_t)sizeof(T), (uint32_t)(n), (uint32_t)sizeof(T), 2, -1, -1, nullptr },
#define SEG_LDS_GET_R(name, T, AS, n) static PLS_HD AS T *name(unsigned char *smem) { constexpr uint32_t o = Table::placed(0).off[Table::i_##name]; return (AS T *)((AS unsigned char *)smem + o); }
#define SEG_LDS_GET_O(name, T, AS, n, first, last, when) SEG_LDS_GET_R(name, T, AS, n)
/* (the one size that varies with n is the chain's T: a region behind it lies that many bytes behind a constant) */
#define SEG_LDS_VAR_BYTES(n) ((uint32_t)SEG_CHAIN_TBYTES(n))
#define SEG_LDS_GET_V(name, T, AS, n) static PLS_HD AS T *name(unsigned char *smem, uint32_t npos) { \
        constexpr uint32_t o = Table::placed(0).off[Table::i_##name] - SEG_LDS_VAR_BYTES(0); \
        static_assert(o + SEG_LDS_VAR_BYTES(60) == Table::placed(60).off[Table::i_##name] && o + SEG_LDS_VAR_BYTES(SEG_CHAIN_CAP + 1) == Table::placed(SEG_CHAIN_CAP + 1).off[Table::i_##name], "the table's offset"); \
        return (AS T *)((AS unsigned char *)smem + o + SEG_LDS_VAR_BYTES(npos)); }
#define SEG_LDS_ALIGN_X(name, bytes) if (i == i_##name) t.align = (bytes);
#define SEG_LDS_UNPAREN(...) __VA_ARGS__
/* Name##Table: the rows (n_regions of them; region(i, n), end(n): n = the chain positions of the row, which only the chain's layout looks at);
 * Name: the accessors.  ALIGN: a list X(region, bytes) of the regions a body accesses with something wider than their element (a 16-byte vector store into
 * 16-bit entries, a 64-bit atomic on a pair of words, a record read through its struct).  HEAD / ARGS: the template header and arguments in parentheses, or () twice. */
#define SEG_LDS_LAYOUT(Name, LIST, ALIGN, HEAD, ARGS) \
    SEG_LDS_UNPAREN HEAD struct Name##Table { \
        enum { LIST(SEG_LDS_ID_R, SEG_LDS_ID_O, SEG_LDS_ID_R, SEG_LDS_ID_R) n_regions }; \
        static constexpr SegLdsRegion row(int i, uint32_t n) { (void)n; const SegLdsRegion all[] = { LIST(SEG_LDS_ROW_R, SEG_LDS_ROW_O, SEG_LDS_ROW_B, SEG_LDS_ROW_R) }; SegLdsRegion t = all[i]; ALIGN(SEG_LDS_ALIGN_X) return t; } \
        static constexpr SegLdsPlaced placed(uint32_t n) { SegLdsRegion t[n_regions] = {}; for (int i = 0; i < n_regions; i++) t[i] = row(i, n); return seg_lds_place(t, n_regions); } \
        static constexpr SegLdsRegion region(int i, uint32_t n = 0) { SegLdsRegion r = row(i, n); const SegLdsPlaced p = placed(n); r.offset = p.off[i]; if (r.count == SEG_LDS_FITS) r.count = p.bytes[i] / r.elem_bytes; return r; } \
        static constexpr uint32_t end(uint32_t n = 0) { return placed(n).end; } \
    }; \
    SEG_LDS_UNPAREN HEAD struct Name { \
        typedef Name##Table SEG_LDS_UNPAREN ARGS Table; \
        static_assert(Table::placed(1).sound && Table::placed(SEG_CHAIN_CAP + 1).sound, #Name ": every region starts on a multiple of its alignment, every overlay lies inside its place"); \
        LIST(SEG_LDS_GET_R, SEG_LDS_GET_O, SEG_LDS_GET_R, SEG_LDS_GET_V) \
    };

#define SEG_LDS_ALIGN_NONE(X)

/* ---- the layouts, one per body ---------------------------------------------------------------------------------------------------------------------------- */

/* seg_enum_body_k<NT, K1> */
#define SEG_LDS_ENUM(R, O, B, V) \
    R(tw, uint32_t, , SEG_TBL_WORDS)                  /* the candidate's decision tables */ \
    R(px, SegPix, , (SEG_L + 1) * 4)                  /* [(SEG_L + 1)][4]: slot 0 = boundary pixel x0-1 */ \
    R(lut, uint32_t, , 512)                           /* the split table */ \
    R(trflag, uint32_t, , 8)                          /* SEG_TF_* */ \
    R(ht, uint32_t, , 4 * SEG_HT)                     /* [4][SEG_HT] hash table: packed state or ~0 */ \
    R(dense, uint16_t, , 4 * SEG_HT)                  /* [4][SEG_HT] slot -> rank among the distinct states */ \
    R(uniq, uint32_t, , 4 * SEG_NSP)                  /* [4][SEG_NSP] the distinct states, packed */ \
    R(res, uint16_t, , 4 * SEG_NSP)                   /* (no body touches it any more: once the exit index of each distinct state; the bytes stay) */ \
    R(lslot, uint16_t, , NT)                          /* (no body touches it any more: once the hash slot of every lane; the bytes stay) */ \
    R(keys, uint32_t, , NT)                           /* [NT] state key of every lane after K1 steps, ~0 = none */
SEG_LDS_LAYOUT(SegLdsEnum, SEG_LDS_ENUM, SEG_LDS_ALIGN_NONE, (template <int NT>), (<NT>))

/* seg_enum_seeded_body<NT> */
#define SEG_LDS_SEEDED(R, O, B, V) \
    R(tw, uint32_t, , SEG_TBL_WORDS) \
    R(px, SegPix, , (SEG_KIN + SEG_L + 1) * 4)        /* [(SEG_KIN + SEG_L + 1)][4]: slot 0 = boundary pixel xs-1 */ \
    R(lut, uint32_t, , 512) \
    R(trflag, uint32_t, , 8)                          /* SEG_TF_* */ \
    R(ht, uint32_t, , 4 * SEG_EH_WORDS)               /* [4][SEG_EH_WORDS] key or ~0 */ \
    R(dense, uint16_t, , 4 * SEG_EH_WORDS)            /* [4][SEG_EH_WORDS] slot -> dense id */ \
    R(uniq, uint32_t, , 4 * SEG_NSP)                  /* [4][SEG_NSP] the entry states (keys) by dense id */ \
    R(keys, uint32_t, , NT)                           /* [NT] */
SEG_LDS_LAYOUT(SegLdsSeeded, SEG_LDS_SEEDED, SEG_LDS_ALIGN_NONE, (template <int NT>), (<NT>))

/* seg_enum_small_body<NT>: NT / (4 * SEG_NSS) segments a workgroup.  Behind what the step loop needs: the state set, its index table, and the STEP TABLES of the
 * workgroup's pixel records -- as many bytes as lie between them and the end of seg_enum_body's layout, so that the launch's bytes (seg_lds_enum_bytes_v) stay what they are.
 * A value of cn costs 2 * NT bytes (what a step from it leaves at every pixel record) and NT / SEG_PL more (the byte it leaves behind a part's last pixel):
 * SEG_SMALL_NCN values of cn fit (seg_small_tables_fit). */
#define SEG_SMALL_KL 256          /* most entries of SegParams::keylut_small the table path takes */
#define SEG_SMALL_ROOM(NT) (SegLdsEnum<NT>::Table::end() - (uint32_t)(SEG_TBL_WORDS * 4 + 512 * 4 + (NT) / (4 * SEG_NSS) * SEG_L * 4 * sizeof(SegPix) + 4 + SEG_NSS * 4 + SEG_SMALL_KL))
#define SEG_SMALL_NCN(NT) (SEG_SMALL_ROOM(NT) / (2u * (NT) + (NT) / SEG_PL))
#define SEG_LDS_SMALL(R, O, B, V) \
    R(tw, uint32_t, , SEG_TBL_WORDS) \
    R(lut, uint32_t, , 512) \
    R(px, SegPix, , NT / (4 * SEG_NSS) * SEG_L * 4)   /* [NSEGS][SEG_L][4] */ \
    R(trflag, uint32_t, , 1)                          /* some pixel is fully transparent */ \
    R(sts, uint32_t, SEG_AS_LDS, SEG_NSS)             /* (table path) SegParams::st_small */ \
    R(ct, uint16_t, SEG_AS_LDS, SEG_SMALL_NCN(NT) * NT)   /* (table path) [2 cmax + 1][NT]: the step of pixel record q from cn (and th = 0): rem + 128 | (thr + 128) << 8, or SEG_SMALL_NONE */ \
    R(kl, uint8_t, SEG_AS_LDS, SEG_SMALL_KL)          /* (table path) SegParams::keylut_small, a byte an entry (255: none) */ \
    R(bk, uint8_t, SEG_AS_LDS, SEG_SMALL_ROOM(NT) - 2u * SEG_SMALL_NCN(NT) * NT)   /* (table path) [2 cmax + 1][NT / SEG_PL]: the byte that step leaves, for a part's last pixel */
SEG_LDS_LAYOUT(SegLdsSmall, SEG_LDS_SMALL, SEG_LDS_ALIGN_NONE, (template <int NT>), (<NT>))
static_assert(SegLdsSmall<512>::Table::end() == SegLdsEnum<512>::Table::end() && SegLdsSmall<1024>::Table::end() == SegLdsEnum<1024>::Table::end(), "the tables of none / up fill what seg_enum_body's layout leaves them, no more");
static_assert(SEG_SMALL_ROOM(512) - 2u * SEG_SMALL_NCN(512) * 512 >= SEG_SMALL_NCN(512) * (512 / SEG_PL) && SEG_SMALL_ROOM(1024) - 2u * SEG_SMALL_NCN(1024) * 1024 >= SEG_SMALL_NCN(1024) * (1024 / SEG_PL), "bk holds a byte per value of cn and part");
/* the table path of seg_enum_small_body: the step tables of a set with |cn| <= cmax, |th| <= tmax fit (and the sentinel of a void step cannot be taken for a value) */
template <int NT> constexpr bool seg_small_tables_fit(int ns, int cmax, int tmax)
{
    return ns > 0 && ns <= SEG_NSS && cmax >= 0 && tmax >= 0 && cmax <= 30 && tmax <= 30 && (uint32_t)(2 * cmax + 1) <= SEG_SMALL_NCN(NT) && (2 * cmax + 1) * (2 * tmax + 1) <= SEG_SMALL_KL;
}

/* seg_enum_unit_body<LANES, UNIT, NC, SEEDS>: tables, split table, the pool, the first records of every pair, bookkeeping -- and ONE place (work) that holds the
 * first phase's scratch (hash tables, per-turn lists, keys: 10 KB; from seeds: the run-in's records and a turn's staged entry maps behind it) and then, for the
 * second phase, the pairs' full pixel records (15.5 KB for the twenty pairs of none / up): 35.8 KB = four workgroups per CU.  (The first version carved both side by
 * side: 52 KB, three per CU, and the CUs' slots, not their issue, set the kernel's time; the second was sized for 1024 threads: 39.9 KB.  Sixteen / twelve pairs of
 * none / up = 32.5 / 28.6 KB = FIVE per CU were measured: 464 / 451 Mpx/s for 32 frames against 465 -- the slots are not what it is short of; the 4 KB less are worth
 * 1.3 %, though: the other launch groups' control, validation and replay workgroups want 37 - 50 KB next to two or three of these.) */
#define SEG_LDS_UNIT_CPR (SEG_UNT / LANES < NC ? SEG_UNT / LANES : NC)      /* pairs per turn of the first phase */
#define SEG_LDS_UNIT(R, O, B, V) \
    R(tw, uint32_t, , SEG_TBL_WORDS) \
    R(lut, uint32_t, , 512) \
    R(pool, uint32_t, , SEG_UPOOL)                    /* [SEG_UPOOL] the distinct states of all pairs, pair behind pair */ \
    R(px1_std, SegPix, , SEG_UNC_SMALL * (SEG_UN_K1MAX + 1))   /* [NC][SEG_UN_K1MAX + 1]: one channel's first records of a pair, slot 0 = the boundary pixel in front of the unit */ \
    R(misc, uint32_t, , 128)                          /* SEG_UM_* */ \
    R(work, unsigned char, , SEG_LDS_FITS) \
    O(ht, uint32_t, , 2 * SEG_UNT, work, work, "in the first phase")   /* [CPR][HT] key or ~0 (this turn) */ \
    B(dense, uint16_t, , 2 * SEG_UNT)                 /* [CPR][HT] slot -> dense id */ \
    B(uniqr, uint32_t, , SEG_UNT)                     /* [CPR][LANES] this turn's distinct states by dense id */ \
    B(keys, uint32_t, , SEG_UNT)                      /* [NT] */ \
    B(px1_seeds, SegPix, , SEEDS ? NC * (SEG_SEED_KMAX + 1) : 0)   /* (SEEDS) [NC][SEG_SEED_KMAX + 1]: the run-in's records, slot 0 = the pixel in front of the run-in */ \
    B(mapl, uint16_t, , SEEDS ? SEG_LDS_UNIT_CPR * 256 : 0)     /* (SEEDS) [CPR][256]: entry index -> dense id of the turn's pairs, staged here and stored coalesced */ \
    O(px, SegPix, , SEG_UNPX, work, work, "in the second phase, behind the barrier that ends the first")   /* [NC][NPX]: all records of a pair */ \
    B(pool2, uint32_t, , SEG_UPOOL)                   /* [SEG_UPOOL] the states that are still distinct behind the unit's first segment, at the pairs' places of the first list */
SEG_LDS_LAYOUT(SegLdsUnit, SEG_LDS_UNIT, SEG_LDS_ALIGN_NONE, (template <int LANES, int UNIT, int NC, bool SEEDS>), (<LANES, UNIT, NC, SEEDS>))

/* seg_first_body<NT, UNITS> */
#define SEG_LDS_FIRST(R, O, B, V) \
    R(tw, uint32_t, , SEG_TBL_WORDS) \
    R(lut, uint32_t, , 512) \
    R(Hf, uint32_t, , 256)                            /* the frozen histogram */ \
    R(rank, uint32_t, , 256) \
    R(px, SegPix, , (UNITS ? SEG_UNIT : 1) * SEG_L * 4)   /* [npix][4]: up to a unit's pixels */
SEG_LDS_LAYOUT(SegLdsFirst, SEG_LDS_FIRST, SEG_LDS_ALIGN_NONE, (template <int NT, bool UNITS>), (<NT, UNITS>))

/* seg_chain_body<SEEDED, CT, UNITS>; n = the chain positions of the widest row of the launch (segments, or units).  Only the seeded instantiation has the repair
 * path and so the tables and pixel records behind T.  (R, the exit states by id of a pass with useR, lies INSIDE T's bytes, behind the rows the pass uses.) */
#define SEG_LDS_CHAIN(R, O, B, V) \
    R(Hf, uint32_t, SEG_AS_LDS, 256)                  /* (repair only) */ \
    R(rank, uint32_t, SEG_AS_LDS, 256)                /* (repair only) */ \
    R(lut, uint32_t, SEG_AS_LDS, 512)                 /* (repair only) */ \
    R(idxb, uint32_t, SEG_AS_LDS, 32)                 /* SEG_CI_* */ \
    R(dn, uint32_t, SEG_AS_LDS, SEG_CHAIN_POS)        /* [SEG_CHAIN_POS] dense id at every position of the pass */ \
    R(entL, uint32_t, SEG_AS_LDS, SEG_CHAIN_POS)      /* [SEG_CHAIN_POS] entry state at every position of the pass (from 1; 0: idxb[SEG_CI_ENTRY0]) */ \
    R(G, uint16_t, SEG_AS_LDS, 2 * SEG_CHAIN_GWORDS)  /* [nblk + 1][stride] composed tables of the blocks */ \
    R(T, uint16_t, SEG_AS_LDS, SEG_CHAIN_TBYTES(n) / 2)   /* [rows][stride]: T[k] takes a dense id of position k to one of position k+1 */ \
    V(twr, uint32_t, SEG_AS_LDS, SEEDED ? SEG_TBL_WORDS : 0)   /* (repair only) the candidate's decision tables */ \
    V(pxr, SegPix, SEG_AS_LDS, SEEDED ? SEG_L + 1 : 0)         /* (repair only) [SEG_L + 1] the walked segment's pixel records */
#define SEG_LDS_CHAIN_ALIGN(X) X(T, 16)           /* the gather stores eight entries at once: *(SegVec16 *)(T + ...) */
SEG_LDS_LAYOUT(SegLdsChain, SEG_LDS_CHAIN, SEG_LDS_CHAIN_ALIGN, (template <bool SEEDED>), (<SEEDED>))

/* seg_extremes_body<CT> */
#define SEG_LDS_EXTREMES(R, O, B, V) \
    R(mm, uint32_t, , 2)                              /* SEG_MM_* */
SEG_LDS_LAYOUT(SegLdsExtremes, SEG_LDS_EXTREMES, SEG_LDS_ALIGN_NONE, (), ())

/* seg_replay_body<RNT> */
#define SEG_LDS_REPLAY(R, O, B, V) \
    R(Hf, uint32_t, , 256) \
    R(rank, uint32_t, , 256) \
    R(lut, uint32_t, , 512) \
    R(tw, uint32_t, , SEG_TBL_WORDS) \
    R(px, SegPix, , SEG_GRP * SEG_L * 4)              /* [SEG_GRP][SEG_L][4] */ \
    R(cnt, uint32_t, , SEG_GRP * 64)                  /* [SEG_GRP][64]: four bins a word (seg_cnt_add) */ \
    R(lane, uint32_t, , SEG_GRP * SEG_PARTS * 4 * 2)  /* [SEG_GRP * SEG_PARTS * 4][2]: start state, first | end pixel << 16 (or ~0: idle) */ \
    R(cwl, uint32_t, , SEG_REPLAY_THREADS * 4)        /* [SEG_REPLAY_THREADS][4] the group's candidate words */ \
    R(oaL, uint32_t, , SEG_REPLAY_THREADS + 3)        /* [SEG_REPLAY_THREADS + 1] the ORIGINAL row above, from the pixel in front of the group; [+1] the original pixel in front of the group, [+2] its new bytes */ \
    O(rm, uint32_t, , 768, tw, tw, "behind the walk")  /* [768] none's bound: largest H0 within reach of a centre value (centre + 256) */ \
    B(red, uint32_t, , 16)                            /* SEG_RR_* */ \
    B(h0s, uint32_t, , 256)                           /* [256] the committed histogram */
#define SEG_LDS_REPLAY_ALIGN(X) X(red, 8)         /* derr and the bound are summed with 64-bit atomics */
SEG_LDS_LAYOUT(SegLdsReplay, SEG_LDS_REPLAY, SEG_LDS_REPLAY_ALIGN, (), ())

/* seg_post_body<VGRP>: 36.9 KB for half replay groups, 51.0 KB for whole ones (round 5: 49 KB before for half groups -- the launch that carries it was short of CUs
 * with that much free next to the enumeration of another launch group) */
#define SEG_LDS_POST(R, O, B, V) \
    R(H0, uint32_t, , 256) \
    R(rank, uint32_t, , 256) \
    R(spare, uint32_t, , 256)                         /* (no body reads it; the bytes stay: they decide how many workgroups share a CU) */ \
    R(cum, uint32_t, , (VGRP + 1) * 256)              /* [VGRP + 1][256]: bumps in front of each segment of the group (staging: row sl + 1 = the bumps OF segment sl) */ \
    R(cw, uint32_t, , (VGRP * SEG_L + 2) * 4)         /* [(NPX + 2)][4] candidate words, from pixel xg0 - 2 */ \
    R(red, uint32_t, , 64)                            /* SEG_PR_* */ \
    R(lut, uint32_t, , 512)                           /* [512] split table */ \
    R(ro, uint32_t, , VGRP * SEG_L + 2)               /* [NPX + 1] original row, from pixel xg0 - 1 */ \
    R(na, uint32_t, , VGRP * SEG_L + 2)               /* [NPX + 1] optimised row above */ \
    R(e0, uint32_t, , 2 * VGRP * SEG_L)               /* [NPX][2] incoming error */ \
    R(wbits, uint32_t, , 32)                          /* SEG_WB_* */ \
    R(slot_of, uint8_t, , 256)                        /* [256] slot of a watched bin or 255 */ \
    R(pend, uint8_t, , VGRP * SEG_L * 4)              /* [NPX * 4] decision waits for pass 3 */ \
    R(binb, uint8_t, , VGRP * SEG_BINB_STRIDE)        /* [VGRP][SEG_BINB_STRIDE] bin of every decision */ \
    R(pcw, uint32_t, , SEG_WATCH_OF(VGRP) * SEG_PC_STRIDE_V(VGRP))   /* [NW][PCS] prefix counts of the watched bins */ \
    R(btop, uint32_t, , 2 * SEG_NBAND * 4)            /* [2][SEG_NBAND][4] */ \
    R(hiG, uint32_t, , 256) \
    R(loG, uint32_t, , 256) \
    O(cumx, uint32_t, , (SEG_GRP - VGRP) * 256, pcw, pcw, "while staging, before pcw is written: barriers lie between")   /* [SEG_GRP - VGRP][256] the bumps of the replay group's segments in front of this half */
SEG_LDS_LAYOUT(SegLdsPost, SEG_LDS_POST, SEG_LDS_ALIGN_NONE, (template <int VGRP>), (<VGRP>))

/* seg_ctl_commit: split table, control block + sums, decision, five tiles, err1 of both parities, spec: 33.8 KB */
#define SEG_LDS_COMMIT(R, O, B, V) \
    R(head, uint32_t, SEG_AS_LDS, 8)                  /* (no body reads it) */ \
    R(lutb, uint32_t, SEG_AS_LDS, 512)                /* [512] next-rows terms of the split */ \
    R(ctlc, uint32_t, SEG_AS_LDS, SEG_CTLC_WORDS)     /* the finished attempt's control block ... */ \
    R(accc, uint32_t, SEG_AS_LDS, SEG_ACCC_WORDS)     /* ... and sums */ \
    R(decision, uint32_t, SEG_AS_LDS, SEG_DEC_WORDS)  /* the SegDecision, shared by the lane that took it */ \
    R(verdict, uint32_t, SEG_AS_LDS, 4 * SEG_NFILT)   /* [SEG_NFILT][4] the candidates' verdicts: cost lo / hi, state, - */ \
    R(ecost, uint32_t, SEG_AS_LDS, 8)                 /* [8] entropy cost of every candidate row */ \
    R(failmask, uint32_t, SEG_AS_LDS, 8)              /* [0] failmask of the attempt two before: which attempt is followed */ \
    R(cw5, uint32_t, SEG_AS_LDS, SEG_NFILT * (SEG_COMMIT_W + 4) * 4)   /* [SEG_NFILT][(SEG_COMMIT_W + 4)][4] every candidate's words of this workgroup's pixels, two more on either side; the winner's become their terms */ \
    R(ext, uint32_t, SEG_AS_LDS, SEG_COMMIT_W * 4)    /* [2][SEG_COMMIT_W][2]: err1 of either row parity (which row is committed is in the control block these loads ride along with) */ \
    R(spec, uint32_t, SEG_AS_LDS, (SEG_NFILT + 1) * 256)   /* [SEG_NFILT + 1][256] the bumps of every candidate's row, the committed histogram (for the row costs: seg_entropy_costs) */
#define SEG_LDS_COMMIT_ALIGN(X) X(ctlc, 8) X(accc, 8)   /* read as SegCtl / SegAcc: 64-bit members */
SEG_LDS_LAYOUT(SegLdsCommit, SEG_LDS_COMMIT, SEG_LDS_COMMIT_ALIGN, (), ())

/* seg_ctl_body<TPARTS>, the candidate workgroups and the image-wide one: four histograms and the table staging area -- stage and stage_cls are ONE run of
 * SEG_TBL_WORDS words to seg_build_tables (pre[2], suf[2], then the classes); until the tables are built, what the decision needs lives below the classes */
#define SEG_LDS_CTL(R, O, B, V) \
    R(Hn, uint32_t, SEG_AS_LDS, 256) \
    R(rank, uint32_t, SEG_AS_LDS, 256) \
    R(scratch, uint32_t, SEG_AS_LDS, 256)             /* (by itself nothing: the place of K's first half and of walk_state) */ \
    R(basen, uint32_t, SEG_AS_LDS, 256) \
    R(stage, uint32_t, SEG_AS_LDS, 4 * SEG_TN)        /* a candidate's tables before they go out */ \
    R(stage_cls, uint32_t, SEG_AS_LDS, SEG_TBL_WORDS - 4 * SEG_TN) \
    O(K, uint64_t, SEG_AS_LDS, 256, scratch, basen, "while seg_build_tables runs: behind basen's last read (the barrier in front of the call)")   /* [256] (H << 32 | rank) of a bin */ \
    O(walk_state, SegState, SEG_AS_LDS, 4, scratch, scratch, "while lane 0 finishes a row serially, in front of seg_build_tables")   /* [4] by channel */ \
    O(spec, uint32_t, SEG_AS_LDS, (SEG_NFILT + 1) * 256, stage, stage, "until the tables are built")   /* [SEG_NFILT + 1][256]: per candidate w, base[w] + every group's bumps of w's row; the committed histogram */ \
    B(ctlc, uint32_t, SEG_AS_LDS, SEG_CTLC_WORDS)     /* the finished attempt's control block and sums, copied by the same burst of loads */ \
    B(accc, uint32_t, SEG_AS_LDS, SEG_ACCC_WORDS) \
    B(decision, uint32_t, SEG_AS_LDS, SEG_DEC_WORDS)  /* as in seg_ctl_commit */ \
    B(verdict, uint32_t, SEG_AS_LDS, 4 * SEG_NFILT) \
    B(ecost, uint32_t, SEG_AS_LDS, 8) \
    B(failmask, uint32_t, SEG_AS_LDS, 4)
#define SEG_LDS_CTL_ALIGN(X) X(ctlc, 8) X(accc, 8) X(walk_state, 4)   /* read as SegCtl / SegAcc: 64-bit members; SegState: three ints */
SEG_LDS_LAYOUT(SegLdsCtl, SEG_LDS_CTL, SEG_LDS_CTL_ALIGN, (), ())

/* ---- the LDS bytes of a launch: the largest end among the bodies its kernel dispatches (pl_seg_launch.h: seg_dispatch_*), plus a pad -------------------------
 * The pads are bytes no body touches.  They stay because the byte count of a launch decides how many workgroups share a CU, and every count here is one a
 * measurement was taken with (SEG_WATCH_OF, SEG_UNT, SEG_REPLAY_NT_BATCH). */
#define SEG_LDS_PAD_ENUM 128
#define SEG_LDS_PAD_UNIT 0
#define SEG_LDS_PAD_CHAIN 64
#define SEG_LDS_PAD_REPLAY 64
#define SEG_LDS_PAD_CTL 256
/* (every count a compile-time value: the launcher asks for them once per attempt) */
/* seg_k_enum<NT>: seg_enum_body, seg_enum_small_body, seg_first_body */
template <int NT> constexpr uint32_t seg_lds_enum_bytes_v = seg_lds_max(SegLdsEnum<NT>::Table::end(), SegLdsSmall<NT>::Table::end(), SegLdsFirst<NT, false>::Table::end()) + SEG_LDS_PAD_ENUM;
constexpr uint32_t seg_lds_enum_bytes(unsigned nt) { return nt == 512 ? seg_lds_enum_bytes_v<512> : seg_lds_enum_bytes_v<1024>; }
/* seg_k_enum_seeded<NT>: seg_enum_seeded_body, seg_first_body */
template <int NT> constexpr uint32_t seg_lds_seeded_bytes_v = seg_lds_max(SegLdsSeeded<NT>::Table::end(), SegLdsFirst<NT, false>::Table::end()) + SEG_LDS_PAD_ENUM;
constexpr uint32_t seg_lds_seeded_bytes(unsigned nt) { return nt == 512 ? seg_lds_seeded_bytes_v<512> : seg_lds_seeded_bytes_v<1024>; }
/* seg_k_enum_unit<UNIT>: seg_enum_unit_body from every state, from seeds and for none / up, seg_first_body.  ONE count for seg_k_enum_unit<SEG_UNIT> and <1>
 * (as before: the place behind the first phase's scratch was sized for the run-in's records of either) */
template <int UNIT> constexpr uint32_t seg_lds_unit_end_v =
    seg_lds_max(SegLdsUnit<SEG_NSP, UNIT, SEG_UNC, false>::Table::end(), SegLdsUnit<SEG_SEED_LANES, UNIT, SEG_UNC_SEEDS_OF(UNIT), true>::Table::end(),
                SegLdsUnit<SEG_NSS, UNIT, SEG_UNC_SMALL_OF(UNIT), false>::Table::end(), SegLdsFirst<SEG_UNT, (UNIT > 1)>::Table::end());
constexpr uint32_t seg_lds_unit_bytes_v = seg_lds_max(seg_lds_unit_end_v<SEG_UNIT>, seg_lds_unit_end_v<1>) + SEG_LDS_PAD_UNIT;
constexpr uint32_t seg_lds_unit_bytes() { return seg_lds_unit_bytes_v; }
/* seg_k_chain<SEEDED, CT, UNITS>: seg_chain_body, seg_extremes_body; n = the chain positions of the launch's widest row (the one run-time count: a constant
 * plus the bytes of T) */
template <bool SEEDED> constexpr uint32_t seg_lds_chain_fixed_v = SegLdsChain<SEEDED>::Table::end(0) - SEG_LDS_VAR_BYTES(0);
template <bool SEEDED> constexpr uint32_t seg_lds_chain_bytes(uint32_t n)
{
    static_assert(seg_lds_chain_fixed_v<SEEDED> + SEG_LDS_VAR_BYTES(60) == SegLdsChain<SEEDED>::Table::end(60) && seg_lds_chain_fixed_v<SEEDED> + SEG_LDS_VAR_BYTES(SEG_CHAIN_CAP + 1) == SegLdsChain<SEEDED>::Table::end(SEG_CHAIN_CAP + 1), "the table's end");
    constexpr uint32_t extremes = SegLdsExtremes::Table::end();
    return seg_lds_max(seg_lds_chain_fixed_v<SEEDED> + SEG_LDS_VAR_BYTES(n), extremes) + SEG_LDS_PAD_CHAIN;
}
/* seg_k_replay<RNT>: seg_replay_body */
constexpr uint32_t seg_lds_replay_bytes_v = SegLdsReplay::Table::end() + SEG_LDS_PAD_REPLAY;
constexpr uint32_t seg_lds_replay_bytes() { return seg_lds_replay_bytes_v; }
/* seg_k_ctl<TPARTS>: seg_ctl_body (which hands the commit workgroups to seg_ctl_commit) and, next to them, the validation seg_post_body<SEG_VGRP_OF(TPARTS)> */
template <int TPARTS> constexpr uint32_t seg_lds_ctl_bytes_v = seg_lds_max(SegLdsCtl::Table::end(), SegLdsCommit::Table::end(), SegLdsPost<SEG_VGRP_OF(TPARTS)>::Table::end()) + SEG_LDS_PAD_CTL;
template <int TPARTS> constexpr uint32_t seg_lds_ctl_bytes() { return seg_lds_ctl_bytes_v<TPARTS>; }

/* (the names the launch tests read) */
#define SEG_SM_ENUM_NT(nt) seg_lds_enum_bytes(nt)
#define SEG_SM_ENUM_SEEDED(nt) seg_lds_seeded_bytes(nt)
#define SEG_SM_ENUM_UNIT seg_lds_unit_bytes()
#define SEG_SM_CHAIN(nseg) seg_lds_chain_bytes<true>((uint32_t)(nseg))
#define SEG_SM_CHAIN_X(npos) seg_lds_chain_bytes<false>((uint32_t)(npos))
#define SEG_SM_REPLAY seg_lds_replay_bytes()
#define SEG_SM_CTLVAL_V(V) ((V) == SEG_VGRP_UNITS ? seg_lds_ctl_bytes<SEG_TPARTS_BATCH>() : seg_lds_ctl_bytes<SEG_TPARTS>())

static_assert(seg_lds_replay_bytes() <= 65536 && seg_lds_enum_bytes(1024) <= 65536 && seg_lds_seeded_bytes(1024) <= 65536 && seg_lds_unit_bytes() <= 65536, "these kernels are launched without an LDS opt-in");

#endif

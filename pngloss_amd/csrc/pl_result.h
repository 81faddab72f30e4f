/*
 * pl_result.h -- the per-image result record (PlJob::result, SegJob::result): PLR_WORDS 32-bit words that the row engines fill on the device and
 * the host reads when the batch is finished.  Internal, not part of the C ABI.
 *
 * Plain C++17 without HIP: the kernels (pl_engine.hip, pl_seg_core.h, pl_rows.hip, pl_prepost.hip), pl_host.hip and the CPU tests
 * (tests/c/result_host.cpp) take every slot number from here, and pl_result_decode below is the one reader of a record.
 *
 * Words 0..4 mean the same for every engine.  The rest is per engine: each engine's slots are listed in a table, and a static_assert proves that
 * no two slots of one engine overlap and that all of them fit the record.  Two engines may use the same word for different things, so the host
 * never asks the record which engine ran an image: the batch plan (pl_plan.h) says so.
 */
#ifndef PL_RESULT_H
#define PL_RESULT_H

#include "../../include/pngloss_hip.h"

#include <stddef.h>
#include <stdint.h>

constexpr int PLR_WORDS = 64;

/* the row engines, as pngloss_hip_last_engine_info reports them in info[PLR_INFO_ENGINE] */
constexpr int PLR_ENGINE_WG = 0;     /* one workgroup per image (pl_engine.hip) */
constexpr int PLR_ENGINE_SEG = 3;    /* segment-parallel (pl_seg.hip) */
constexpr int PLR_ENGINE_ROWS = 4;   /* row statistics, strength 0 (pl_rows.hip) */

/* ---- every engine ---- */
constexpr int PLR_STATUS = 0;        /* PNGLOSS_SUCCESS, or the device status of an abort */
constexpr int PLR_BPP = 1;
constexpr int PLR_UNIQUE = 2;        /* non-zero bins of the final histogram */
constexpr int PLR_RETRIED = 3;       /* rows that needed the strength-decrement retry */
constexpr int PLR_REPAIRED = 4;      /* pngloss_hip_result::repaired_pixels: workgroup engine: pixels chain wave 0 redid exactly; segment engine: epochs */

/* ---- workgroup engine (the pl_engine.hip epilogue; kilo-cycles = cycles >> 10).  Chain wave w runs candidate row w: up, sub, average, paeth, none ---- */
constexpr int PLR_WG_WAVES = 5;             /* chain waves */
constexpr int PLR_WG_LEAD_ROWS = 5;         /* row attempts on the band-leader chains */
constexpr int PLR_WG_RESCANS = 6;           /* band rescans of wave 0 */
constexpr int PLR_WG_SIMD_MAP = 7;          /* the SIMD of waves 0..7, two bits each */
constexpr int PLR_WG_CHAIN_KCYC = 8;        /* [PLR_WG_CHAIN_WAVES] kilo-cycles in the serial chain per chain wave */
constexpr int PLR_WG_CHAIN_WAVES = 4;       /* (waves 0..3; wave 4 has the PLR_WG_W4_* slots) */
constexpr int PLR_WG_SLOW_PX = 12;          /* [PLR_WG_CHAIN_WAVES] pixels that needed the exact repair per chain wave */
constexpr int PLR_WG_LIGHT_PX = 16;         /* [PLR_WG_WAVES] light pixels per chain wave */
constexpr int PLR_WG_ADAPT_LEGACY = 21;     /* rows on the round-1 chains by the adaptive choice */
constexpr int PLR_WG_EST_LEAD = 22;         /* last cycles per pixel: band-leader chains */
constexpr int PLR_WG_EST_LEGACY = 23;       /* ... round-1 chains */
constexpr int PLR_WG_W4_KCYC = 24;          /* wave 4: kilo-cycles in the serial chain */
constexpr int PLR_WG_W4_SLOW_PX = 25;       /* ... exact redos */
constexpr int PLR_WG_W4_RESCANS = 26;       /* ... band rescans */
constexpr int PLR_WG_FLUSH_KCYC = 27;       /* [PLR_WG_WAVES] kilo-cycles of flush + relation check per chain wave */
constexpr int PLR_WG_PHASE_KCYC = 32;       /* [PLR_WG_WAVES][PLR_WG_PHASES] kilo-cycles per chain wave: vector, fast groups, exact redo, rescan, table build */
constexpr int PLR_WG_PHASES = 5;
constexpr int PLR_WG_CYC_PER_PX = 57;       /* [PLR_WG_WAVES] cycles per pixel of undisturbed whole-chunk runs */
constexpr int PLR_WG_POST_KCYC = 62;        /* wave 0: kilo-cycles in the post pass */
constexpr int PLR_WG_COMMIT_KCYC = 63;      /* ... in the commit pass */

/* ---- segment engine (pl_seg_core.h).  The control kernel's epilogue writes the fields.  The phase clocks (100 MHz ticks) are written only when
 *      PNGLOSS_HIP_SEGPROF sets SegParams::engine_flags bit 0: the slowest workgroup (_MAX), the sum over the workgroups (_SUM), their count (_RUNS) ---- */
constexpr int PLR_SEG_ATTEMPTS = 5;         /* row attempts */
constexpr int PLR_SEG_SERIAL_ROWS = 6;      /* rows finished serially */
constexpr int PLR_SEG_NONE_DROPPED = 7;     /* rows in which candidate none was ruled out by its cost bound */
constexpr int PLR_SEG_FIELDS_END = 8;       /* (the control kernel's epilogue always clears the words below this) */
/* chain kernel: gather, compose, walk, tail (it clocks the first three) */
constexpr int PLR_SEG_CHAIN_MAX = 8;        /* [PLR_SEG_CHAIN_PHASES] */
constexpr int PLR_SEG_CHAIN_SUM = 12;       /* [PLR_SEG_CHAIN_PHASES] */
constexpr int PLR_SEG_CHAIN_PHASES = 4;
constexpr int PLR_SEG_CHAIN_RUNS = 16;
constexpr int PLR_SEG_WALKED = 17;          /* segments walked step by step by the chain kernel (counted with or without the clocks) */
constexpr int PLR_SEG_CHAIN_WIDE = 18;      /* chain runs at the wide stride */
/* control kernel, candidate workgroups: requests + copy, decision, new histogram + fields; commit workgroups: requests + copy */
constexpr int PLR_SEG_CAND_REQ_SUM = 19;
constexpr int PLR_ENGINE_ID = 20;           /* PLR_ENGINE_SEG / PLR_ENGINE_ROWS, stored by those engines' kernels: the host does not read it */
constexpr int PLR_SEG_CAND_DECIDE_SUM = 21;
constexpr int PLR_SEG_CAND_HIST_SUM = 22;
constexpr int PLR_SEG_COMMIT_REQ_SUM = 23;
constexpr int PLR_SEG_LOW_CLOCKS_END = 24;  /* (the epilogue clears the clocks below this, PLR_SEG_WALKED excepted, when they are off) */
/* enumeration: load, first steps + dedupe, remaining steps, map */
constexpr int PLR_SEG_ENUM_MAX = 24;        /* [PLR_SEG_ENUM_PHASES] */
constexpr int PLR_SEG_ENUM_SUM = 28;        /* [PLR_SEG_ENUM_PHASES] */
constexpr int PLR_SEG_ENUM_PHASES = 4;
constexpr int PLR_SEG_ENUM_RUNS = 32;
constexpr int PLR_SEG_ENUM_STATES = 33;     /* distinct states of the four channels after the dedupe, summed over the runs */
/* first-segment walker */
constexpr int PLR_SEG_FIRST_MAX = 34;
constexpr int PLR_SEG_FIRST_SUM = 35;
constexpr int PLR_SEG_FIRST_RUNS = 36;
/* table build: keys, classes, entries + write (its runs are PLR_SEG_CAND_RUNS) */
constexpr int PLR_SEG_TABLE_SUM = 37;       /* [PLR_SEG_TABLE_PHASES] */
constexpr int PLR_SEG_TABLE_PHASES = 3;
/* validation: load, pass1, watched bins + pass3, none bound, sums */
constexpr int PLR_SEG_VAL_MAX = 40;         /* [PLR_SEG_VAL_PHASES] */
constexpr int PLR_SEG_VAL_PHASES = 5;
constexpr int PLR_SEG_COMMIT_DECIDE_SUM = 45;
constexpr int PLR_SEG_VAL_PENDING = 46;     /* pending decisions (pass 3) */
constexpr int PLR_SEG_VAL_SUM = 48;         /* [PLR_SEG_VAL_PHASES] */
constexpr int PLR_SEG_VAL_RUNS = 53;
/* control kernel, commit workgroups: terms, rows + extremes; whole workgroups */
constexpr int PLR_SEG_COMMIT_TERMS_SUM = 54;
constexpr int PLR_SEG_COMMIT_ROWS_SUM = 55;
constexpr int PLR_SEG_CTL_MAX = 56;         /* [PLR_SEG_CTL_PARTS] candidate workgroup up to the table build, table build, commit workgroup */
constexpr int PLR_SEG_CTL_PARTS = 3;
constexpr int PLR_SEG_CAND_SUM = 59;        /* [2] candidate workgroup up to the table build, table build */
constexpr int PLR_SEG_CAND_RUNS = 61;
constexpr int PLR_SEG_COMMIT_SUM = 62;
constexpr int PLR_SEG_COMMIT_RUNS = 63;

/* ---- row-statistics engine (pl_rows.hip): clears the record, then the words of every engine (PLR_REPAIRED stays 0), PLR_ENGINE_ID and ---- */
constexpr int PLR_ROWS_ROWS = 5;            /* "row attempts": one per row */

/* ---- the layout, checked: every slot or range an engine writes, no two overlapping, all inside the record ---- */
struct PlrRange { int base, count; };
template <size_t N>
constexpr bool plr_disjoint(const PlrRange (&r)[N])
{
    for (size_t a = 0; a < N; a++) {
        if (r[a].base < 0 || r[a].count < 1 || r[a].base + r[a].count > PLR_WORDS) return false;
        for (size_t b = a + 1; b < N; b++)
            if (r[a].base < r[b].base + r[b].count && r[b].base < r[a].base + r[a].count) return false;
    }
    return true;
}
#define PLR_COMMON_RANGES { PLR_STATUS, 1 }, { PLR_BPP, 1 }, { PLR_UNIQUE, 1 }, { PLR_RETRIED, 1 }, { PLR_REPAIRED, 1 }
constexpr PlrRange PLR_LAYOUT_WG[] = {
    PLR_COMMON_RANGES, { PLR_WG_LEAD_ROWS, 1 }, { PLR_WG_RESCANS, 1 }, { PLR_WG_SIMD_MAP, 1 }, { PLR_WG_CHAIN_KCYC, PLR_WG_CHAIN_WAVES },
    { PLR_WG_SLOW_PX, PLR_WG_CHAIN_WAVES }, { PLR_WG_LIGHT_PX, PLR_WG_WAVES }, { PLR_WG_ADAPT_LEGACY, 1 }, { PLR_WG_EST_LEAD, 1 }, { PLR_WG_EST_LEGACY, 1 },
    { PLR_WG_W4_KCYC, 1 }, { PLR_WG_W4_SLOW_PX, 1 }, { PLR_WG_W4_RESCANS, 1 }, { PLR_WG_FLUSH_KCYC, PLR_WG_WAVES },
    { PLR_WG_PHASE_KCYC, PLR_WG_WAVES * PLR_WG_PHASES }, { PLR_WG_CYC_PER_PX, PLR_WG_WAVES }, { PLR_WG_POST_KCYC, 1 }, { PLR_WG_COMMIT_KCYC, 1 },
};
constexpr PlrRange PLR_LAYOUT_SEG[] = {
    PLR_COMMON_RANGES, { PLR_SEG_ATTEMPTS, 1 }, { PLR_SEG_SERIAL_ROWS, 1 }, { PLR_SEG_NONE_DROPPED, 1 },
    { PLR_SEG_CHAIN_MAX, PLR_SEG_CHAIN_PHASES }, { PLR_SEG_CHAIN_SUM, PLR_SEG_CHAIN_PHASES }, { PLR_SEG_CHAIN_RUNS, 1 }, { PLR_SEG_WALKED, 1 },
    { PLR_SEG_CHAIN_WIDE, 1 }, { PLR_SEG_CAND_REQ_SUM, 1 }, { PLR_ENGINE_ID, 1 }, { PLR_SEG_CAND_DECIDE_SUM, 1 }, { PLR_SEG_CAND_HIST_SUM, 1 },
    { PLR_SEG_COMMIT_REQ_SUM, 1 }, { PLR_SEG_ENUM_MAX, PLR_SEG_ENUM_PHASES }, { PLR_SEG_ENUM_SUM, PLR_SEG_ENUM_PHASES }, { PLR_SEG_ENUM_RUNS, 1 },
    { PLR_SEG_ENUM_STATES, 1 }, { PLR_SEG_FIRST_MAX, 1 }, { PLR_SEG_FIRST_SUM, 1 }, { PLR_SEG_FIRST_RUNS, 1 }, { PLR_SEG_TABLE_SUM, PLR_SEG_TABLE_PHASES },
    { PLR_SEG_VAL_MAX, PLR_SEG_VAL_PHASES }, { PLR_SEG_COMMIT_DECIDE_SUM, 1 }, { PLR_SEG_VAL_PENDING, 1 }, { PLR_SEG_VAL_SUM, PLR_SEG_VAL_PHASES },
    { PLR_SEG_VAL_RUNS, 1 }, { PLR_SEG_COMMIT_TERMS_SUM, 1 }, { PLR_SEG_COMMIT_ROWS_SUM, 1 }, { PLR_SEG_CTL_MAX, PLR_SEG_CTL_PARTS },
    { PLR_SEG_CAND_SUM, 2 }, { PLR_SEG_CAND_RUNS, 1 }, { PLR_SEG_COMMIT_SUM, 1 }, { PLR_SEG_COMMIT_RUNS, 1 },
};
constexpr PlrRange PLR_LAYOUT_ROWS[] = { PLR_COMMON_RANGES, { PLR_ROWS_ROWS, 1 }, { PLR_ENGINE_ID, 1 } };
#undef PLR_COMMON_RANGES
static_assert(plr_disjoint(PLR_LAYOUT_WG), "workgroup engine: result slots overlap or leave the record");
static_assert(plr_disjoint(PLR_LAYOUT_SEG), "segment engine: result slots overlap or leave the record");
static_assert(plr_disjoint(PLR_LAYOUT_ROWS), "row-statistics engine: result slots overlap or leave the record");
static_assert(PLR_SEG_FIELDS_END == PLR_SEG_NONE_DROPPED + 1 && PLR_SEG_FIELDS_END == PLR_SEG_CHAIN_MAX && PLR_SEG_LOW_CLOCKS_END == PLR_SEG_ENUM_MAX,
              "the bounds of the segment engine's clearing rule");

/* ---- pngloss_hip_last_engine_info(ctx, index, info[PLR_INFO_WORDS]) ---- */
constexpr int PLR_INFO_ENGINE = 0;
constexpr int PLR_INFO_ATTEMPTS = 1;
constexpr int PLR_INFO_RESTARTS = 2;
constexpr int PLR_INFO_SERIAL_ROWS = 3;
constexpr int PLR_INFO_NONE_DROPPED = 4;
constexpr int PLR_INFO_WALKED = 5;
constexpr int PLR_INFO_LAUNCH_GROUPS = 6;   /* (fields of the context, not of the record: the caller's) */
constexpr int PLR_INFO_STREAM_WAIT = 7;
constexpr int PLR_INFO_WORDS = 8;

/* The one reader of a record r[PLR_WORDS].  engine (PLR_ENGINE_*): the engine the batch plan gave the image.  Fills the image's result and its
 * engine_info words; info[PLR_INFO_LAUNCH_GROUPS] and info[PLR_INFO_STREAM_WAIT] are left 0 for the caller. */
inline void pl_result_decode(const int32_t *r, int engine, pngloss_hip_result *res, int32_t *info)
{
    *res = pngloss_hip_result{ r[PLR_STATUS], (uint32_t)r[PLR_BPP], (uint32_t)r[PLR_UNIQUE], (uint32_t)r[PLR_RETRIED], (uint32_t)r[PLR_REPAIRED] };
    for (int i = 0; i < PLR_INFO_WORDS; i++) info[i] = 0;
    info[PLR_INFO_ENGINE] = engine;
    if (engine == PLR_ENGINE_SEG) {
        info[PLR_INFO_ATTEMPTS] = r[PLR_SEG_ATTEMPTS]; info[PLR_INFO_RESTARTS] = r[PLR_REPAIRED]; info[PLR_INFO_SERIAL_ROWS] = r[PLR_SEG_SERIAL_ROWS];
        info[PLR_INFO_NONE_DROPPED] = r[PLR_SEG_NONE_DROPPED]; info[PLR_INFO_WALKED] = r[PLR_SEG_WALKED];
    } else if (engine == PLR_ENGINE_ROWS) {
        info[PLR_INFO_ATTEMPTS] = r[PLR_ROWS_ROWS];
    } else {
        info[PLR_INFO_ATTEMPTS] = r[PLR_WG_LEAD_ROWS]; info[PLR_INFO_RESTARTS] = r[PLR_REPAIRED]; info[PLR_INFO_SERIAL_ROWS] = r[PLR_WG_ADAPT_LEGACY];
    }
}

#endif

/*
 * seg_host.cpp -- TEST INFRASTRUCTURE: runs the kernel bodies of the segment-parallel row engine
 * (pngloss_amd/csrc/pl_seg_core.h, the same source hipcc compiles into pl_seg.hip's kernels) on the CPU, as plain loops
 * over (workgroup, thread) -- the launches of an attempt, their grids and what each workgroup does are the shipped library's own
 * (pngloss_amd/csrc/pl_seg_launch.h) --, so that the CPU suite can check the engine's logic bit-exactly against the oracle without a GPU.
 * Never shipped, never loaded by the product (which has no CPU path).
 *
 *   seg_host_optimize(rgba, W, H, row_filters|NULL, strength, bleed, stats[8])  -> 0, or 64 if (strength, bleed) has more
 *   chain states than the enumeration has lanes (the product then uses the one-workgroup-per-image engine)
 */
static unsigned long long seg_dbg[4][2];   /* [slot]: events, sum */
#define SEG_DEBUG_COUNT(slot, v) (seg_dbg[slot][0]++, seg_dbg[slot][1] += (v))
/* per row: which candidates went through an epoch (failed validation) or an extra start, and who won */
static unsigned seg_row_mask, seg_row_none;
static unsigned long long seg_epochs[5], seg_epoch_rows[5], seg_epoch_rows_won[5], seg_none_starts, seg_none_started_won, seg_rows;
static void seg_debug_row(int kind, unsigned failed, int winner, int start_none)
{
    if (kind == 1) { for (int f = 0; f < 5; f++) if ((failed >> f) & 1u) { seg_epochs[f]++; seg_row_mask |= 1u << f; } if (start_none) { seg_none_starts++; seg_row_none = 1; } }
    if (kind == 3) {
        seg_rows++;
        for (int f = 0; f < 5; f++) if ((seg_row_mask >> f) & 1u) { seg_epoch_rows[f]++; if (winner == f) seg_epoch_rows_won[f]++; }
        if (seg_row_none && winner == 0) seg_none_started_won++;
        seg_row_mask = 0; seg_row_none = 0;
    }
}
#define SEG_DEBUG_ROW(kind, failed, winner, start_none) seg_debug_row((kind), (failed), (winner), (start_none))
#include <cstdio>
#include <cstdlib>
#define SEG_DEBUG_BREAK(f, c, sg, est, y) do { if (getenv("SEG_HOST_VERBOSE") && atoi(getenv("SEG_HOST_VERBOSE")) > 1) fprintf(stderr, "seg_host: row %u broken off: candidate %d channel %d segment %u, entry state left %u cn %d th %d\n", (unsigned)(y), (int)(f), (int)(c), (unsigned)(sg), (unsigned)((est) & 255u), (int)(((est) >> 8) & 0xffffu) - 32768, (int)((est) >> 24) - 128); } while (0)
#include "../../pngloss_amd/csrc/pl_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

int paeth_i(int a, int d, int l) { return seg_paeth(a, d, l); }

struct Arena {
    std::vector<std::vector<unsigned char>> bufs;
    template <class T> T *take(size_t n) { bufs.emplace_back((n ? n : 1) * sizeof(T) + 64, (unsigned char)0xA5); return (T *)bufs.back().data(); }   /* junk-filled: nothing may rely on zeroed memory */
    /* the engine's own arrays: a block of exactly `bytes` (none at all for an empty array), so that the sanitizers see the first byte behind what the library allocates */
    std::vector<std::unique_ptr<unsigned char[]>> exact;
    unsigned char *take_exact(size_t bytes) { exact.emplace_back(new unsigned char[bytes]); std::memset(exact.back().get(), 0xA5, bytes); return exact.back().get(); }
};

} // namespace

/* what the engine does with a (strength, bleed) pair: out = { supported, seeded, chain states (exhaustive), run-in pixels, cmax, tmax, dmax, seeds of none / up } */
extern "C" int seg_host_describe(unsigned strength, long bleed, int32_t *out)
{
    static SegParams P;
    const bool ok = seg_build_params(P, (int)strength, (int)bleed);
    out[0] = ok; out[1] = P.seeded; out[2] = P.ns; out[3] = P.kin; out[4] = P.cmax; out[5] = P.tmax; out[6] = P.dmax; out[7] = P.nseed_small;
    return ok ? 0 : 64;
}

/* the seed set of the unit enumeration from seeds (round 6): out = { seed_n, seed_kin, ns, dmax }, states[i] = (delta, cn, th) of seed i */
extern "C" int seg_host_seeds(unsigned strength, long bleed, int32_t *out, int32_t *states)
{
    static SegParams P;
    if (!seg_build_params(P, (int)strength, (int)bleed)) return 64;
    out[0] = P.seed_n; out[1] = P.seed_kin; out[2] = P.ns; out[3] = P.dmax;
    for (int i = 0; i < P.seed_n; i++) {
        if (P.seed_idx[i] >= P.ns) return 65;
        const uint32_t w = P.st_pack[P.seed_idx[i]];
        states[3 * i] = (int)(w & 255u) - 128; states[3 * i + 1] = (int)((w >> 8) & 255u) - 128; states[3 * i + 2] = (int)((w >> 16) & 255u) - 128;
    }
    return 0;
}

extern "C" int seg_host_optimize(unsigned char *rgba, uint32_t W, uint32_t H, unsigned char *row_filters, unsigned strength, long bleed, uint32_t *stats)
{
    if (!W || !H) return 0;
    static SegParams P;
    if (!seg_build_params(P, (int)strength, (int)bleed, getenv("SEG_HOST_SEEDED") != nullptr)) return 64;
    if (getenv("SEG_HOST_FORCE_FILTER")) P.engine_flags = (atoi(getenv("SEG_HOST_FORCE_FILTER")) + 1) << 8;
    if (getenv("SEG_HOST_FLAGS")) P.engine_flags |= atoi(getenv("SEG_HOST_FLAGS")) & 0xfe;   /* test hooks of the chain kernel (2: slow path, 4: wide stride) */
    if (getenv("SEG_HOST_UNIT") && atoi(getenv("SEG_HOST_UNIT")) && !P.seeded && (P.ns <= SEG_NSP || atoi(getenv("SEG_HOST_UNIT")) > 1)) { P.unit = SEG_UNIT; P.tparts = SEG_TPARTS_BATCH; }
    if (getenv("SEG_HOST_TPARTS")) P.tparts = atoi(getenv("SEG_HOST_TPARTS")) == 1 ? SEG_TPARTS_BATCH : SEG_TPARTS;   /* enumeration in units, as the launcher asks for batches (seg_enum_unit_body) */
    /* classify + pack into slots (what pl_classify / pl_repack do on the device) */
    bool gray = true, opaque = true;
    for (size_t i = 0; i < (size_t)W * H; i++) { const unsigned char *p = rgba + 4 * i; gray &= p[0] == p[1] && p[1] == p[2]; opaque &= p[3] == 255; }
    const uint32_t bpp = gray ? (opaque ? 1u : 2u) : (opaque ? 3u : 4u);
    Arena A;
    uint32_t *img = A.take<uint32_t>((size_t)W * H);
    for (size_t i = 0; i < (size_t)W * H; i++) {
        const unsigned char *p = rgba + 4 * i;
        img[i] = bpp == 4 ? ((uint32_t)p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24)) : bpp == 3 ? ((uint32_t)p[0] | (p[1] << 8) | (p[2] << 16))
                 : bpp == 2 ? ((uint32_t)p[1] | (p[3] << 8)) : (uint32_t)p[1];
    }
    /* original_frequency + ranks (pl_hist / pl_rank) */
    std::vector<uint32_t> oh(5 * 256, 0), rank(5 * 256, 0);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++)
            for (uint32_t c = 0; c < bpp; c++) {
                auto at = [&](long yy, long xx) -> int { return (yy < 0 || xx < 0) ? 0 : (int)((img[(size_t)yy * W + xx] >> (8 * c)) & 255u); };
                const int hv = at(y, x), lv = at(y, (long)x - 1), av = at((long)y - 1, x), dv = at((long)y - 1, (long)x - 1);
                oh[0 * 256 + (hv & 255)]++; oh[1 * 256 + ((hv - lv) & 255)]++; oh[2 * 256 + ((hv - av) & 255)]++;
                oh[3 * 256 + ((hv - ((av + lv) >> 1)) & 255)]++; oh[4 * 256 + ((hv - paeth_i(av, dv, lv)) & 255)]++;
            }
    for (int f = 0; f < 5; f++) for (int b = 0; b < 256; b++) { uint32_t r = 0; for (int k = 0; k < 256; k++) r += oh[f * 256 + k] < oh[f * 256 + b]; rank[f * 256 + b] = r; }

    SegJob j{};
    j.img = img; j.W = W; j.H = H; j.bpp = bpp;
    j.row_filters = row_filters;
    j.row_ids = A.take<uint8_t>(H);
    j.orig_rank = rank.data();
    j.cand = A.take<uint32_t>((size_t)5 * W * 4);
    j.final_hist = A.take<uint32_t>(256); j.result = A.take<int32_t>(PLR_WORDS); j.progress = nullptr;
    if (W > SEG_MAX_WIDTH) return 64;
    /* the workspace of the image as the library lays it out (pl_seg_layout: its sizes, not the harness's own), every array a heap block of its own */
    pl_seg_bind(j, pl_seg_layout(W ? W : 1, (uint32_t)P.nsp, P.seeded != 0), W, [&](const PlSegArray &a) { return A.take_exact(a.bytes); });
    j.nbreak = 0u;
    j.self = &j; for (int k = 0; k < 3; k++) { j.v[k].magic = 0u; j.v[k].finished = 0u; j.v[k].ignore = 0u; j.vfail[k] = 0u; }
    j.ctl[2].magic = 0u; j.acc[2].failmask = 0u;   /* (seg_k_resolve does this on the device: the first attempt finds no attempt behind it) */
    /* the shape of the attempts (pl_plan_batch fills it for a launch group): this image's own, or -- SEG_HOST_GRID_PAD=k -- that of a group whose widest image has k
     * segments more, which is what a batch does to its narrower images: every grid then has workgroups without work */
    const uint32_t pad = getenv("SEG_HOST_GRID_PAD") ? (uint32_t)atoi(getenv("SEG_HOST_GRID_PAD")) : 0u;
    SegShape shape{};
    shape.max_nseg = j.nseg + pad; shape.max_ngrp = (shape.max_nseg + SEG_GRP - 1) / SEG_GRP; shape.max_ncommit = (W + pad * SEG_L + SEG_COMMIT_W - 1) / SEG_COMMIT_W;
    /* the enumeration's workgroups come in two sizes; the product picks by row width, SEG_HOST_ENUM_NT pins one */
    shape.enum_nt = shape.max_nseg <= SEG_ENUM_NT_SMALL_MAX_NSEG ? 512 : 1024;
    if (getenv("SEG_HOST_ENUM_NT")) shape.enum_nt = atoi(getenv("SEG_HOST_ENUM_NT")) == 1024 ? 1024 : 512;
    shape.tparts = (uint32_t)P.tparts; shape.unit = (uint32_t)P.unit; shape.small_ok = P.small_ok != 0; shape.seeded = P.seeded != 0;
    /* the start from seeds with a run-in (round 6): units, or (unit = 1) segment by segment through the same bodies */
    shape.seeds = !P.seeded && P.ns <= SEG_NSP && P.seed_n > 0 && getenv("SEG_HOST_SEEDS") != nullptr && atoi(getenv("SEG_HOST_SEEDS")) != 0;
    if (shape.seeds && getenv("SEG_HOST_SEED_KIN")) P.seed_kin = atoi(getenv("SEG_HOST_SEED_KIN"));
    SegLaunch launches[SEG_MAX_LAUNCHES];
    const int nl = seg_attempt_launches(shape, launches);
    int attempt = 0;
    const long max_attempts = pl_seg_max_attempts(H, (int)strength);
    /* One attempt = the four or five launches of seg_attempt_launches: [control of this attempt + validation of the attempt before], enumerate, (seeded sets: gather,)
     * chain, replay; every workgroup of every grid, each launch with a buffer of exactly its LDS request (the sanitizer build, tests/test_seg_host.py, sees any
     * byte beyond it).  The two halves of the first launch run side by side on the device; here one after the other, in either order (SEG_HOST_VAL_FIRST):
     * neither may depend on it. */
    const bool val_first = getenv("SEG_HOST_VAL_FIRST") != nullptr;
    for (;; attempt++) {
        if (attempt > max_attempts) { fprintf(stderr, "seg_host: no progress\n"); return 65; }
        const int par = attempt % 3;
        for (int i = 0; i < nl; i++) {
            const SegLaunch &L = launches[i];
            std::vector<unsigned char> smem(L.lds_bytes, 0x5A);
            auto run = [&](unsigned from, unsigned to) { for (unsigned bx = from; bx < to; bx++) seg_dispatch_block(L, j, P, par, bx, smem.data()); };
            if (i == 0 && val_first) { run(L.a, L.grid_x); run(0, L.a); }      /* (L.a: the control workgroups of the first launch, the validation's behind them) */
            else run(0, L.grid_x);
            if (i == 0 && j.ctl[par].finished == 2u) break;
        }
        if (j.ctl[par].finished == 2u) break;
    }
    const SegCtl &fc = j.ctl[attempt % 3];
    if (getenv("SEG_HOST_VERBOSE")) {
        fprintf(stderr, "seg_host: %llu rows; epochs per candidate (none sub up avg paeth): %llu %llu %llu %llu %llu; rows with an epoch of it: %llu %llu %llu %llu %llu, of which it won: %llu %llu %llu %llu %llu; extra starts of none %llu (won %llu)\n",
                seg_rows, seg_epochs[0], seg_epochs[1], seg_epochs[2], seg_epochs[3], seg_epochs[4], seg_epoch_rows[0], seg_epoch_rows[1], seg_epoch_rows[2], seg_epoch_rows[3], seg_epoch_rows[4],
                seg_epoch_rows_won[0], seg_epoch_rows_won[1], seg_epoch_rows_won[2], seg_epoch_rows_won[3], seg_epoch_rows_won[4], seg_none_starts, seg_none_started_won);
    }
    if (getenv("SEG_HOST_VERBOSE")) fprintf(stderr, "seg_host: replay lanes from an entry state %llu (%.1f px each), from a checkpoint %llu (%.1f px each)\n", seg_dbg[0][0], seg_dbg[0][0] ? (double)seg_dbg[0][1] / seg_dbg[0][0] : 0.0, seg_dbg[1][0], seg_dbg[1][0] ? (double)seg_dbg[1][1] / seg_dbg[1][0] : 0.0);
    if (getenv("SEG_HOST_VERBOSE")) fprintf(stderr, "seg_host: chain repairs (segments walked step by step) %llu\n", seg_dbg[2][0]);
    if (stats) { stats[0] = (uint32_t)attempt; stats[1] = fc.restarts_total; stats[2] = fc.retried; stats[3] = fc.serial_rows; stats[4] = (uint32_t)j.result[PLR_UNIQUE]; stats[5] = bpp; stats[6] = (uint32_t)P.ns; stats[7] = fc.status; }
    /* unpack (pl_unpack) */
    for (size_t i = 0; i < (size_t)W * H; i++) {
        unsigned char *p = rgba + 4 * i; const uint32_t w = img[i];
        switch (bpp) {
        case 1: p[0] = p[1] = p[2] = (unsigned char)w; p[3] = 255; break;
        case 2: p[0] = p[1] = p[2] = (unsigned char)w; p[3] = (unsigned char)(w >> 8); break;
        case 3: p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = 255; break;
        default: p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = (unsigned char)(w >> 24); break;
        }
    }
    return (int)fc.status;
}

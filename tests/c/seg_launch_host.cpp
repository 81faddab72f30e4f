/*
 * seg_launch_host.cpp -- TEST INFRASTRUCTURE: the shape of a row attempt of the segment engine (pngloss_amd/csrc/pl_seg_launch.h, the header pl_seg.hip
 * carries out) behind a thin C ABI, so that the CPU suite pins every grid, workgroup size, LDS request and scalar argument, and checks what the workgroups
 * of those grids do (tests/test_seg_launch_host.py).  The dispatch functions are compiled with RECORDING STUBS in the kernel bodies' place (SEG_BODY): a
 * stub writes down which body it stands for, its template arguments and what it was called with.
 *
 *   seg_launch_host_constants(out[48]) -> how many        the SEG_* constants the test's restatement of the launcher needs, in the order of NAMES there
 *   seg_launch_host_sm_chain(n, x)                         SEG_SM_CHAIN(n) (x = 0) or SEG_SM_CHAIN_X(n)
 *   seg_launch_host_launches(shape[9], out[5][7]) -> n     shape: max_nseg, max_ngrp, max_ncommit, enum_nt, tparts, unit, small_ok, seeded, seeds;
 *                                                          out: kernel id, grid_x, threads, lds_bytes, a, b, seeds
 *   seg_launch_host_visit(shape[9], par, img[5 + 5], out[cap][8], cap) -> records
 *       img: W, bpp, seed_n, nbreak, y, start_x[5] of an image of the launch group; every workgroup of every launch of the attempt is dispatched;
 *       out: launch, body, template arguments (2 words), par, and the body's three arguments (f, .., ..; unused ones 0)
 */
#include <cstdint>
#include <vector>

struct SegJob;
struct SegParams;
struct SegCtlView;
namespace seg_stub {
struct Rec { int32_t launch, body, t0, t1, par, a, b, c; };
static std::vector<Rec> *sink;
static int launch;
static void put(int body, int t0, int t1, int par, int a, int b, int c) { sink->push_back(Rec{ launch, body, t0, t1, par, a, b, c }); }
enum { CTL, POST, ENUM, ENUM_SMALL, FIRST, ENUM_SEEDED, ENUM_UNIT, GATHER, EXTREMES, CHAIN, REPLAY };
template <int TPARTS> void seg_ctl_body(const SegJob &, const SegParams &, int par, int bx, unsigned char *) { put(CTL, TPARTS, 0, par, bx, 0, 0); }
template <int VGRP> void seg_post_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int vg, unsigned char *) { put(POST, VGRP, 0, par, f, vg, 0); }
template <int NT> void seg_enum_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int seg, int chalf, unsigned char *) { put(ENUM, NT, 0, par, f, seg, chalf); }
template <int NT> void seg_enum_small_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int seg0, unsigned char *) { put(ENUM_SMALL, NT, 0, par, f, seg0, 0); }
template <int NT, bool UNITS> void seg_first_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, unsigned char *) { put(FIRST, NT, UNITS, par, f, 0, 0); }
template <int NT> void seg_enum_seeded_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int seg, int chalf, unsigned char *) { put(ENUM_SEEDED, NT, 0, par, f, seg, chalf); }
template <int LANES, int UNIT, int NC, bool SEEDS = false> void seg_enum_unit_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int grp, unsigned char *) { put(ENUM_UNIT, LANES, (UNIT * 1000 + NC) * 2 + SEEDS, par, f, grp, 0); }
inline void seg_gather_seeded_body(const SegJob &, const SegCtlView &, int f, int c, int blk) { put(GATHER, 0, 0, -1, f, c, blk); }
template <int CT> void seg_extremes_body(const SegJob &, const SegParams &, const SegCtlView &, int par, unsigned char *) { put(EXTREMES, CT, 0, par, 0, 0, 0); }
template <bool SEEDED, int CT, bool UNITS> void seg_chain_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int c, unsigned char *) { put(CHAIN, CT, SEEDED * 2 + UNITS, par, f, c, 0); }
template <int RNT> void seg_replay_body(const SegJob &, const SegParams &, const SegCtlView &, int par, int f, int grp, unsigned char *) { put(REPLAY, RNT, 0, par, f, grp, 0); }
}
#define SEG_BODY(name) seg_stub::name
#include "../../pngloss_amd/csrc/pl_seg_launch.h"

static SegShape shape_of(const int64_t *s)
{
    SegShape h{};
    h.max_nseg = (uint32_t)s[0]; h.max_ngrp = (uint32_t)s[1]; h.max_ncommit = (uint32_t)s[2]; h.enum_nt = (uint32_t)s[3]; h.tparts = (uint32_t)s[4]; h.unit = (uint32_t)s[5];
    h.small_ok = s[6] != 0; h.seeded = s[7] != 0; h.seeds = s[8] != 0;
    return h;
}

extern "C" {

int seg_launch_host_constants(int64_t *out)
{
    const int64_t v[] = {
        SEG_NFILT, SEG_TPARTS, SEG_TPARTS_BATCH, SEG_GRP, SEG_VGRP_OF(SEG_TPARTS), SEG_VGRP_OF(SEG_TPARTS_BATCH), SEG_THREADS,
        (int64_t)SEG_SM_CTLVAL_V(SEG_VGRP_OF(SEG_TPARTS)), (int64_t)SEG_SM_CTLVAL_V(SEG_VGRP_OF(SEG_TPARTS_BATCH)), SEG_NSP, SEG_NSS, SEG_UNIT, SEG_UNC, SEG_UNC_SEEDS, SEG_UNC_SEEDS1,
        SEG_UNC_SMALL, SEG_UNC_SMALL_OF(1), SEG_UNT, SEG_SM_ENUM_UNIT, SEG_SM_ENUM_NT(512), SEG_SM_ENUM_NT(1024), SEG_SM_ENUM_SEEDED(512), SEG_SM_ENUM_SEEDED(1024),
        SEG_GS, SEG_GT, SEG_CHAIN_THREADS, SEG_CHAIN_THREADS_UNIT, SEG_REPLAY_NT, SEG_REPLAY_NT_BATCH, SEG_SM_REPLAY, SEG_ENUM_NT_SMALL_MAX_NSEG, SEG_CHAIN_CAP8, SEG_CHAIN_CAP,
        SEG_L, SEG_COMMIT_W, SEG_EXPERIMENT_NO_VAL_CODE, SEG_SEED_LANES,
        SEG_KERNEL_CTL, SEG_KERNEL_CTL_BATCH, SEG_KERNEL_ENUM_512, SEG_KERNEL_ENUM_1024, SEG_KERNEL_ENUM_SEEDED_512, SEG_KERNEL_ENUM_SEEDED_1024, SEG_KERNEL_ENUM_UNIT, SEG_KERNEL_ENUM_UNIT1,
        SEG_KERNEL_GATHER_SEEDED, SEG_KERNEL_CHAIN, SEG_KERNEL_CHAIN_SEEDED, SEG_KERNEL_CHAIN_UNIT, SEG_KERNEL_REPLAY, SEG_KERNEL_REPLAY_BATCH, SEG_MAX_LAUNCHES,
    };
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; i++) out[i] = v[i];
    return n;
}

int64_t seg_launch_host_sm_chain(int64_t n, int x) { return x ? (int64_t)SEG_SM_CHAIN_X(n) : (int64_t)SEG_SM_CHAIN(n); }

int seg_launch_host_launches(const int64_t *shape, int64_t *out)
{
    SegLaunch L[SEG_MAX_LAUNCHES];
    const int n = seg_attempt_launches(shape_of(shape), L);
    for (int i = 0; i < n; i++) {
        const int64_t v[7] = { L[i].kernel, L[i].grid_x, L[i].threads, (int64_t)L[i].lds_bytes, L[i].a, L[i].b, L[i].seeds };
        for (int k = 0; k < 7; k++) out[7 * i + k] = v[k];
    }
    return n;
}

int64_t seg_launch_host_visit(const int64_t *shape, int par, const int64_t *img, int32_t *out, int64_t cap)
{
    const SegShape h = shape_of(shape);
    static SegParams P;
    P = SegParams{};
    P.small_ok = h.small_ok; P.seeded = h.seeded; P.unit = (int32_t)h.unit; P.tparts = (int32_t)h.tparts; P.seed_n = (int32_t)img[2];
    SegJob j{};
    j.W = (uint32_t)img[0]; j.bpp = (uint32_t)img[1]; j.nbreak = (uint32_t)img[3];
    j.nseg = (j.W + SEG_L - 1) / SEG_L; j.ngrp = (j.nseg + SEG_GRP - 1) / SEG_GRP;
    for (int k = 0; k < 3; k++) {
        j.v[k].magic = SEG_MAGIC; j.v[k].y = (uint32_t)img[4];
        for (int f = 0; f < SEG_NFILT; f++) { j.v[k].active[f] = 1u; j.v[k].start_x[f] = (uint32_t)img[5 + f]; }
    }
    std::vector<seg_stub::Rec> recs;
    seg_stub::sink = &recs;
    SegLaunch L[SEG_MAX_LAUNCHES];
    const int n = seg_attempt_launches(h, L);
    for (int i = 0; i < n; i++) {
        seg_stub::launch = i;
        for (unsigned bx = 0; bx < L[i].grid_x; bx++) seg_dispatch_block(L[i], j, P, par, bx, nullptr);
    }
    seg_stub::sink = nullptr;
    for (size_t r = 0; r < recs.size() && (int64_t)r < cap; r++) {
        const seg_stub::Rec &q = recs[r];
        const int32_t v[8] = { q.launch, q.body, q.t0, q.t1, q.par, q.a, q.b, q.c };
        for (int k = 0; k < 8; k++) out[8 * r + k] = v[k];
    }
    return (int64_t)recs.size();
}

} /* extern "C" */

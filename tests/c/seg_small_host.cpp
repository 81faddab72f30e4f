/*
 * seg_small_host.cpp -- TEST INFRASTRUCTURE: the enumeration body of none / up (pngloss_amd/csrc/pl_seg_core.h: seg_enum_small_body) with its TABLE PATH checked against
 * its step loop, workgroup by workgroup, inside whole images run by the CPU harness (tests/c/seg_host.cpp, which this file includes: the launches, grids and LDS bytes are
 * the shipped library's own).  Never shipped.
 *
 * Every call of the body the launches make lands in seg_small_hook, which
 *   mode 0  runs the body as shipped (the table path wherever the set's tables fit), then the body with the step loop alone (TABLES = false) on the same job, and compares
 *           every record either leaves in the places the workgroup may write -- maps, dcnt, rck, rout, rst, junk-filled before each run, so that a record one of them
 *           leaves out counts too -- and then puts back what was there and runs the body as shipped once more: the image goes on with the shipped body's records;
 *   mode 1  runs the step loop alone: the body of the parent commit.
 *   mode 2  like mode 0, but the two runs that are compared see an incoming-error row with +-90 in every plane of two pixels in five: next to bytes near 0 or 255 the band
 *           is clamped, the diff passes the strength, and cn leaves -cmax .. cmax in mid-segment (and comes back within a few pixels) -- which the engine's own error rows
 *           never do on the suite's images.  The row is put back before the run that stays; counts[3], counts[4] then count the lanes of the perturbed runs.
 *   seg_small_host_run(rgba, W, H, row_filters|NULL, strength, bleed, mode, stats[8], counts[8]) -> seg_host_optimize's status;
 *   counts = { calls of the body, records that differ, lanes that walked their tables, lanes of the table path that ran the loop, of these: back in the set at the segment's end,
 *              lanes of a body without tables, ns_small, 1 if the set's tables fit the enumeration's workgroups of the image }
 * Built by tests/test_seg_small_host.py as a shared object and, with -DSEG_SMALL_MAIN and -fsanitize=address,undefined, as a program of its own (main below).
 */
#include <cstdint>
struct SegJob; struct SegParams; struct SegCtlView;
template <int NT> inline void seg_small_hook(const SegJob &j, const SegParams &P, const SegCtlView &cv, int par, int f, int seg0, unsigned char *smem);
#define SEG_BODY(name) SEG_BODY_##name
#define SEG_BODY_seg_ctl_body seg_ctl_body
#define SEG_BODY_seg_post_body seg_post_body
#define SEG_BODY_seg_enum_body seg_enum_body
#define SEG_BODY_seg_enum_small_body seg_small_hook
#define SEG_BODY_seg_first_body seg_first_body
#define SEG_BODY_seg_enum_seeded_body seg_enum_seeded_body
#define SEG_BODY_seg_enum_unit_body seg_enum_unit_body
#define SEG_BODY_seg_gather_seeded_body seg_gather_seeded_body
#define SEG_BODY_seg_extremes_body seg_extremes_body
#define SEG_BODY_seg_chain_body seg_chain_body
#define SEG_BODY_seg_replay_body seg_replay_body
static unsigned long long small_counts[8];
static void small_count_lane(bool tables, bool walked, uint32_t out)
{
    if (!tables) small_counts[5]++;
    else if (walked) small_counts[2]++;
    else { small_counts[3]++; if (out != 0xFFFFu) small_counts[4]++; }
}
#define SEG_DEBUG_SMALL(tables, walked, out) small_count_lane((tables), (walked), (out))

#include "seg_host.cpp"

static int small_mode;
static unsigned long long small_perturbed[2];

namespace {
/* the places a workgroup of the body may write: SEG_NSS lanes of every channel of its segments */
struct SmallRecords {
    std::vector<uint32_t> w;
    bool operator==(const SmallRecords &o) const { return w == o.w; }
};
template <class FN> void small_each(const SegJob &j, const SegParams &P, int f, int seg0, int nsegs, FN fn)
{
    for (uint32_t seg = (uint32_t)seg0; seg < (uint32_t)(seg0 + nsegs) && seg < j.nseg; seg++)
        for (int c = 0; c < 4; c++) {
            const size_t base = ((size_t)f * j.nseg + seg) * 4 + c;
            fn(j.dcnt[base]);
            for (int i = 0; i < SEG_NSS; i++) {
                const size_t slot = base * SEG_NSP + i;
                fn(j.maps[base * (size_t)P.nsp + i]); fn(j.rout[slot]); fn(j.rst[slot]);
                for (int k = 0; k < SEG_PARTS - 1; k++) fn(j.rck[slot * (SEG_PARTS - 1) + k]);
            }
        }
}
SmallRecords small_take(const SegJob &j, const SegParams &P, int f, int seg0, int nsegs)
{
    SmallRecords r;
    small_each(j, P, f, seg0, nsegs, [&](auto &x) { r.w.push_back((uint32_t)x); });
    return r;
}
void small_put(const SegJob &j, const SegParams &P, int f, int seg0, int nsegs, const SmallRecords &r)
{
    size_t k = 0;
    small_each(j, P, f, seg0, nsegs, [&](auto &x) { x = (typename std::remove_reference<decltype(x)>::type)r.w[k++]; });
}
void small_junk(const SegJob &j, const SegParams &P, int f, int seg0, int nsegs)
{
    small_each(j, P, f, seg0, nsegs, [&](auto &x) { x = (typename std::remove_reference<decltype(x)>::type)0xDEADBEEFu; });
}
} // namespace

template <int NT> inline void seg_small_hook(const SegJob &j, const SegParams &P, const SegCtlView &cv, int par, int f, int seg0, unsigned char *smem)
{
    constexpr int NSEGS = NT / (4 * SEG_NSS);
    const size_t lds = seg_lds_enum_bytes(NT);
    if (small_mode == 1) { seg_enum_small_body<NT, false>(j, P, cv, par, f, seg0, smem); return; }
    small_counts[0]++;
    unsigned long long keep[8];
    memcpy(keep, small_counts, sizeof keep);
    const SmallRecords before = small_take(j, P, f, seg0, NSEGS);
    std::vector<uint32_t> e0_keep;
    uint32_t *e0 = seg_e0(j, cv.y);
    if (small_mode == 2 && !cv.finished && cv.active == 1) {
        e0_keep.assign(e0, e0 + 2 * (size_t)j.W);
        for (uint32_t x = (uint32_t)seg0 * SEG_L; x < (uint32_t)(seg0 + NSEGS) * SEG_L && x < j.W; x++) {
            const uint32_t v = x % 5 == 2 ? 90u : (x % 5 == 4 ? (uint32_t)(-90) & 0xffffu : 0u);
            if (v) e0[2 * (size_t)x] = e0[2 * (size_t)x + 1] = v | v << 16;
        }
    }
    small_junk(j, P, f, seg0, NSEGS);
    memset(smem, 0x5A, lds);
    seg_enum_small_body<NT>(j, P, cv, par, f, seg0, smem);
    const SmallRecords shipped = small_take(j, P, f, seg0, NSEGS);
    if (small_mode == 2) { small_perturbed[0] += small_counts[3] - keep[3]; small_perturbed[1] += small_counts[4] - keep[4]; }
    small_junk(j, P, f, seg0, NSEGS);
    memset(smem, 0xC3, lds);
    seg_enum_small_body<NT, false>(j, P, cv, par, f, seg0, smem);
    const SmallRecords loop = small_take(j, P, f, seg0, NSEGS);
    memcpy(small_counts, keep, sizeof keep);          /* (the lanes are counted once, in the run that stays) */
    if (!e0_keep.empty()) memcpy(e0, e0_keep.data(), e0_keep.size() * sizeof(uint32_t));
    for (size_t k = 0; k < loop.w.size(); k++) if (shipped.w[k] != loop.w[k]) small_counts[1]++;
    small_put(j, P, f, seg0, NSEGS, before);
    memset(smem, 0x5A, lds);
    seg_enum_small_body<NT>(j, P, cv, par, f, seg0, smem);
}

extern "C" int seg_small_host_run(unsigned char *rgba, uint32_t W, uint32_t H, unsigned char *row_filters, unsigned strength, long bleed, int mode, uint32_t *stats, uint64_t *counts)
{
    memset(small_counts, 0, sizeof small_counts);
    small_perturbed[0] = small_perturbed[1] = 0;
    small_mode = mode;
    const int rc = seg_host_optimize(rgba, W, H, row_filters, strength, bleed, stats);
    static SegParams P;
    if (seg_build_params(P, (int)strength, (int)bleed, getenv("SEG_HOST_SEEDED") != nullptr)) {
        const uint32_t nseg = (W + SEG_L - 1) / SEG_L;
        bool nt512 = nseg <= SEG_ENUM_NT_SMALL_MAX_NSEG;
        if (getenv("SEG_HOST_ENUM_NT")) nt512 = atoi(getenv("SEG_HOST_ENUM_NT")) != 1024;
        small_counts[6] = (unsigned long long)P.ns_small;
        small_counts[7] = P.small_ok && (nt512 ? seg_small_tables_fit<512>(P.ns_small, P.cmax, P.tmax) : seg_small_tables_fit<1024>(P.ns_small, P.cmax, P.tmax)) ? 1u : 0u;
    }
    if (mode == 2) { small_counts[3] = small_perturbed[0]; small_counts[4] = small_perturbed[1]; }
    if (counts) for (int k = 0; k < 8; k++) counts[k] = small_counts[k];
    return rc;
}

/* ns_small, small_ok and whether the tables fit a workgroup of 512 / 1024 threads, for a (strength, bleed) pair: out[4] */
extern "C" int seg_small_host_describe(unsigned strength, long bleed, int32_t *out)
{
    static SegParams P;
    if (!seg_build_params(P, (int)strength, (int)bleed)) return 64;
    out[0] = P.ns_small; out[1] = P.small_ok; out[2] = P.small_ok && seg_small_tables_fit<512>(P.ns_small, P.cmax, P.tmax); out[3] = P.small_ok && seg_small_tables_fit<1024>(P.ns_small, P.cmax, P.tmax);
    return 0;
}

#ifdef SEG_SMALL_MAIN
/* the program of its own (sanitizers): the generator's frames at the smallest shapes at which the body can go wrong -- widths around one segment, the four segments of a
 * workgroup of 512 threads and the eight of one of 1024, heights 4 .. 6, every byte-per-pixel class and fully transparent pixels, with and without row filters, both sizes
 * of the enumeration's workgroups, the (strength, bleed) pairs given on the command line (all 80 cases, or every n-th of them) -- table path against loop call by call, bytes and filter IDs against the
 * restatement, attempts against the run with the loop alone.  One line per case. */
#include "../../oracle/pngloss_port.h"
extern "C" void pngloss_synth_rgba(unsigned char *rgba, uint32_t width, uint32_t height, int mode, uint64_t frame);
int main(int argc, char **argv)
{
    static const uint32_t widths[] = { 1, 31, 32, 33, 127, 128, 129, 257 };
    static const int modes[] = { 0, 2, 3, 4, 5 };
    int bad = 0, k = 0;
    /* arguments: triples strength bleed every -- the pair, and that it takes every `every`-th of the 80 cases */
    for (int a = 1; a + 2 < argc; a += 3) {
        const unsigned s = (unsigned)atoi(argv[a]); const long b = atol(argv[a + 1]);
        const int every = atoi(argv[a + 2]) > 0 ? atoi(argv[a + 2]) : 1;
        int nth = 0;
        for (uint32_t w : widths)
            for (int mode : modes)
                for (int nt = 512; nt <= 1024; nt += 512) {
                    const uint32_t h = 4 + (uint32_t)(k % 3);
                    const bool ids = ((k++ / 3) & 1) != 0;
                    if (nth++ % every) continue;
                    setenv("SEG_HOST_ENUM_NT", nt == 512 ? "512" : "1024", 1);
                    std::vector<unsigned char> img((size_t)w * h * 4), got, loop, gf(h, 0), lf(h, 0), wf(h, 0);
                    pngloss_synth_rgba(img.data(), w, h, mode, (uint64_t)k);
                    got = img; loop = img;
                    uint32_t st0[8] = {}, st1[8] = {};
                    uint64_t cnt[8] = {}, cnt1[8] = {};
                    const int rc = seg_small_host_run(got.data(), w, h, ids ? gf.data() : nullptr, s, b, 0, st0, cnt);
                    const int rc1 = seg_small_host_run(loop.data(), w, h, ids ? lf.data() : nullptr, s, b, 1, st1, cnt1);
                    std::vector<unsigned char *> rows(h);
                    for (uint32_t y = 0; y < h; y++) rows[y] = img.data() + (size_t)y * w * 4;
                    const int prc = port_optimize_with_rows(rows.data(), w, h, ids ? wf.data() : nullptr, false, (uint_fast8_t)s, (int_fast16_t)b);
                    const bool same = rc == 0 && rc1 == 0 && prc == 0 && got == img && loop == img && gf == wf && lf == wf && st0[0] == st1[0] && cnt[1] == 0;
                    std::printf("%u x %u mode %d nt %d strength %u bleed %ld filters %d: %s attempts %u loop %u calls %llu differ %llu walked %llu fell %llu returned %llu loop_lanes %llu ns_small %llu fits %llu\n",
                                w, h, mode, nt, s, b, (int)ids, same ? "equal" : "DIFFERENT", st0[0], st1[0], (unsigned long long)cnt[0], (unsigned long long)cnt[1], (unsigned long long)cnt[2],
                                (unsigned long long)cnt[3], (unsigned long long)cnt[4], (unsigned long long)cnt[5], (unsigned long long)cnt[6], (unsigned long long)cnt[7]);
                    if (!same) bad++;
                }
    }
    return bad ? 1 : 0;
}
#endif

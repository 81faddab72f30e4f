/* tests/c/dither_host.cpp -- test infrastructure: the error diffusion of pngloss_amd/csrc/pl_dither_core.h run on the CPU in the order pl_dither.hip
 * runs it -- band by band, epoch by epoch, wave by wave, the lanes of a wave as a loop in lock-step --, under the sanitizers.  The waves of an
 * epoch run concurrently on the device; here they run one after the other, ascending or descending, and both orders have to give the same image.
 * The rings and the error line start out poisoned, so that a slot read before it was written shows in the pixels.
 * usage: dither_host constants                     prints "lanes waves band k lag ring"
 *        dither_host run cases.bin out.bin
 *          cases.bin: u32 n; per case u32 width, height, entries, descending; `entries` palette words; width * height u32 words
 *          out.bin:   per case width * height u32 words, then u32 barriers (of every wave), i32 smallest a_c, i32 largest a_c
 *        dither_host sched max_width max_height    the schedule arithmetic for every width in 1 .. max_width and height in 1 .. max_height, as
 *                                                  intervals of columns per lane and epoch: prints "ok <cases> <bands checked>" or the first fault
 *        dither_host barriers w h [w h ...]        prints plf_barriers per pair
 *        dither_host layout base job_bytes w ...   prints "name offset bytes" per region of pl_dither_layout, then "total 0 bytes" */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <tuple>
#include <vector>

#include "../../pngloss_amd/csrc/pl_layout.h"

namespace {

constexpr uint32_t kPoison = 0x7FFF7FFFu;

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

struct Ran { uint64_t barriers; int32_t a_min, a_max; bool ok; };

/* pl_dither's body for one image */
Ran run_image(const uint32_t *img, uint32_t *out, uint32_t W, uint32_t H, const std::vector<uint32_t> &pal, bool descending)
{
    Ran ran = { 0, 0, 255, true };
    std::vector<uint32_t> pal2(2 * PLQ_MAX_COLORS, 0);
    for (uint32_t e = 0; e < pal.size(); e++) { pal2[2 * e] = pal[e]; pal2[2 * e + 1] = plq_base(pal[e], e); }
    const uint32_t entries = (uint32_t)pal.size();
    const PlfErr zero = { 0u, 0u }, poison = { kPoison, kPoison };
    std::vector<PlfErr> ring(PLF_RING_ENTRIES, poison), line(W ? W : 1, poison);
    uint64_t barriers[PLF_WAVES] = {};
    const uint64_t wave_epochs = plf_wave_epochs(W);
    const uint32_t bands = plf_bands(H);
    for (uint32_t band = 0; band < bands; band++) {
        const uint32_t rows = plf_band_rows(H, band), waves = plf_band_waves(rows);
        const uint64_t epochs = plf_band_epochs(W, waves);
        std::vector<PlfLane> lanes((size_t)PLF_WAVES * PLF_LANES, PlfLane{ zero, zero, zero, zero });
        for (uint64_t g = 0; g < epochs; g++) {
            for (uint32_t turn = 0; turn < PLF_WAVES; turn++) {
                const uint32_t wave = descending ? PLF_WAVES - 1 - turn : turn;
                barriers[wave]++;
                const int64_t le = plf_local_epoch(g, wave);
                if (!(wave < waves && le >= 0 && (uint64_t)le < wave_epochs)) continue;
                const bool from_ring = wave > 0, from_line = wave == 0 && band > 0;
                const bool to_ring = wave + 1 < PLF_WAVES, to_line = !to_ring && band + 1 < bands;
                auto above = [&](uint64_t c) -> PlfErr {
                    if (c >= W) return zero;
                    if (from_ring) return ring[plf_ring_index(wave, c)];
                    if (from_line) return line[c];
                    return zero;
                };
                PlfLane *s = lanes.data() + (size_t)wave * PLF_LANES;
                uint64_t t = (uint64_t)le * PLF_K;
                if (le == 0) s[0].ur = above(0);
                for (uint32_t i = 0; i < PLF_K; i++, t++) {
                    PlfErr fetch[PLF_LANES];                                    /* the cross-lane move: every lane reads before any lane writes */
                    for (uint32_t lane = 0; lane < PLF_LANES; lane++) fetch[lane] = lane ? s[lane - 1].last : above(t + 1);
                    for (uint32_t lane = 0; lane < PLF_LANES; lane++) {
                        const int64_t x = plf_column(t, lane);
                        const uint32_t row = wave * PLF_LANES + lane;
                        plf_lane_shift(s[lane], fetch[lane]);
                        if (row < rows && x >= 0 && (uint64_t)x < W) {
                            const size_t at = ((size_t)band * PLF_BAND + row) * W + (size_t)x;
                            int32_t a[4];
                            if (out[at] != kPoison) ran.ok = false;             /* (visited twice) */
                            out[at] = plf_pixel(pal2.data(), entries, img[at], s[lane].last, s[lane].ul, s[lane].up, s[lane].ur, &s[lane].last, a);
                            for (int32_t v : a) { ran.a_min = std::min(ran.a_min, v); ran.a_max = std::max(ran.a_max, v); }
                            if (lane == PLF_LANES - 1) {
                                if (to_ring) ring[plf_ring_index(wave + 1, (uint64_t)x)] = s[lane].last;
                                else if (to_line) line[(size_t)x] = s[lane].last;
                            }
                        } else {
                            s[lane].last = zero;
                        }
                    }
                }
            }
        }
    }
    ran.barriers = barriers[0];
    for (uint64_t b : barriers) if (b != barriers[0]) ran.ok = false;
    if (ran.barriers != plf_barriers(W, H)) ran.ok = false;
    return ran;
}

int run_cases(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!read_u32(in, &ncases, 1)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t head[4];
        if (!read_u32(in, head, 4)) return 3;
        const uint32_t W = head[0], H = head[1], entries = head[2];
        if (entries < 1 || entries > PLQ_MAX_COLORS) return 3;
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> pal(entries), img(n ? n : 1), res(n ? n : 1, kPoison);
        if (!read_u32(in, pal.data(), entries) || (n && !read_u32(in, img.data(), n))) return 3;
        const Ran ran = run_image(img.data(), res.data(), W, H, pal, head[3] != 0);
        if (!ran.ok) { fprintf(stderr, "case %u: a pixel visited twice, or the waves disagree about the barriers\n", c); return 4; }
        fwrite(res.data(), sizeof(uint32_t), n, out);
        const uint32_t tail[3] = { (uint32_t)ran.barriers, (uint32_t)ran.a_min, (uint32_t)ran.a_max };
        fwrite(tail, sizeof tail, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 6;
}

/* ---- the schedule as intervals: what a lane covers in an epoch is the columns of its first to its last local step, cut to the image ---- */

#define FAULT(...) do { fprintf(stdout, __VA_ARGS__); fprintf(stdout, " (width %u, rows %u, first %d, next %d, epoch %llu, wave %u, lane %u)\n", W, rows, (int)first, (int)has_next, (unsigned long long)g, wave, lane); return false; } while (0)

/* one band of `rows` rows; first: no band above it; has_next: a band below it (the last row writes the error line) */
bool check_band(uint32_t W, uint32_t rows, bool first, bool has_next, uint64_t *epochs_out)
{
    const uint32_t waves = plf_band_waves(rows);
    const uint64_t epochs = plf_band_epochs(W, waves), wave_epochs = plf_wave_epochs(W);
    *epochs_out = epochs;
    thread_local int64_t prog[PLF_BAND], prev[PLF_BAND];            /* the next column of a row: now, and when the epoch began (kept for row 0 and every wave's last row) */
    thread_local int64_t lo[PLF_BAND], hi[PLF_BAND];                 /* what the row covers in this epoch (lo > hi: nothing) */
    std::fill(prog, prog + PLF_BAND, 0);
    uint64_t barriers[PLF_WAVES] = {};
    bool works[PLF_WAVES] = {};
    uint64_t g = 0;
    uint32_t wave = 0, lane = 0;
    for (g = 0; g < epochs; g++) {
        prev[0] = prog[0];
        for (wave = 0; wave < waves; wave++) prev[std::min(wave * PLF_LANES + PLF_LANES, rows) - 1] = prog[std::min(wave * PLF_LANES + PLF_LANES, rows) - 1];
        for (wave = 0; wave < PLF_WAVES; wave++) {
            barriers[wave]++;
            const int64_t le = plf_local_epoch(g, wave);
            works[wave] = wave < waves && le >= 0 && (uint64_t)le < wave_epochs;
            if (!works[wave]) continue;
            for (lane = 0; lane < PLF_LANES && wave * PLF_LANES + lane < rows; lane++) {
                const uint32_t row = wave * PLF_LANES + lane;
                lo[row] = 0; hi[row] = -1;
                const uint64_t t0 = (uint64_t)le * PLF_K, t1 = t0 + PLF_K - 1;
                lo[row] = std::max<int64_t>(plf_column(t0, lane), 0);
                hi[row] = std::min<int64_t>(plf_column(t1, lane), (int64_t)W - 1);
                if (lo[row] > hi[row]) continue;
                if (lo[row] != prog[row]) FAULT("a row skips or repeats columns: at %lld, continues at %lld", (long long)prog[row], (long long)lo[row]);
                prog[row] = hi[row] + 1;
                if (lane && plf_column(t0, lane - 1) - plf_column(t0, lane) < 2) FAULT("the lane above is not two columns ahead");
            }
        }
        /* every pixel (y, x) of this epoch behind (y-1, x+1) */
        for (wave = 0; wave < waves; wave++) {
            if (!works[wave]) continue;
            for (lane = 0; lane < PLF_LANES && wave * PLF_LANES + lane < rows; lane++) {
                const uint32_t row = wave * PLF_LANES + lane;
                if (lo[row] > hi[row] || row == 0) continue;
                const int64_t need = std::min<int64_t>(hi[row] + 2, W);            /* the row above has to be here */
                if (lane) {                                         /* the same wave, in lock-step: it is there within the epoch */
                    if (prog[row - 1] < need) FAULT("the lane above has not finished column x+1");
                    continue;
                }
                /* the wave above: only what it had finished when the epoch began counts */
                if (prev[row - 1] < need) FAULT("the wave above had not finished column x+1 when the epoch began");
                /* the ring: the columns read are lo+1 .. need-1 (and column 0 with the first step); they were written (above), and the writer, at
                 * prog[row - 1] when this epoch ends, has not yet written a column that lies PLF_RING behind one of them */
                const int64_t first_read = lo[row] ? lo[row] + 1 : 0;
                if (first_read + (int64_t)PLF_RING < prog[row - 1]) FAULT("a ring slot is overwritten before its reader has passed it");
                if (plf_ring_index(wave, (uint64_t)first_read) / PLF_RING != wave) FAULT("a ring index outside the wave's ring");
            }
        }
        /* the error line: with a band above and a band below, the last row writes where row 0 reads -- only columns row 0 has read before this epoch */
        if (!first && has_next && rows == PLF_BAND && works[PLF_WAVES - 1] && lo[rows - 1] <= hi[rows - 1] && hi[rows - 1] > prev[0]) {
            wave = PLF_WAVES - 1; lane = PLF_LANES - 1;
            FAULT("the error line is overwritten before row 0 of the band has read it");
        }
    }
    wave = lane = 0;
    for (uint32_t row = 0; row < rows; row++)
        if (prog[row] != (int64_t)W) FAULT("row %u ends at column %lld", row, (long long)prog[row]);
    for (uint64_t b : barriers) if (b != epochs) FAULT("a wave counts other barriers");
    if (has_next && rows != PLF_BAND) FAULT("a band that is not full has a band below");
    return true;
}

/* the widths first, first + stride, ...: the widths are independent, a few host threads share them */
int check_widths(uint32_t first, uint32_t stride, uint32_t max_w, uint32_t max_h, uint64_t *cases_out, uint64_t *checked_out)
{
    uint64_t cases = 0, checked = 0;
    for (uint32_t W = first; W <= max_w; W += stride) {
        std::map<std::tuple<uint32_t, bool, bool>, uint64_t> seen;          /* a band's schedule depends on these alone: each is walked once per width */
        for (uint32_t H = 1; H <= max_h; H++, cases++) {
            const uint32_t bands = plf_bands(H);
            uint64_t total = 0, covered = 0;
            for (uint32_t band = 0; band < bands; band++) {
                const uint32_t rows = plf_band_rows(H, band);
                const auto key = std::make_tuple(rows, band == 0, band + 1 < bands);
                auto it = seen.find(key);
                if (it == seen.end()) {
                    uint64_t epochs = 0;
                    if (!check_band(W, rows, band == 0, band + 1 < bands, &epochs)) return 1;
                    it = seen.emplace(key, epochs).first;
                    checked++;
                }
                total += it->second;
                covered += rows;
            }
            if (covered != H) { printf("the bands of height %u hold %llu rows\n", H, (unsigned long long)covered); return 1; }
            if (total != plf_barriers(W, H)) { printf("plf_barriers(%u, %u) = %llu, the bands count %llu\n", W, H, (unsigned long long)plf_barriers(W, H), (unsigned long long)total); return 1; }
        }
    }
    *cases_out = cases;
    *checked_out = checked;
    return 0;
}

int check_schedules(uint32_t max_w, uint32_t max_h)
{
    constexpr uint32_t kTeam = 8;
    uint64_t cases[kTeam] = {}, checked[kTeam] = {};
    int rc[kTeam] = {};
    std::vector<std::thread> team;
    for (uint32_t t = 0; t < kTeam; t++) team.emplace_back([&, t] { rc[t] = check_widths(1 + t, kTeam, max_w, max_h, &cases[t], &checked[t]); });
    for (auto &th : team) th.join();
    uint64_t all = 0, bands = 0;
    for (uint32_t t = 0; t < kTeam; t++) { if (rc[t]) return rc[t]; all += cases[t]; bands += checked[t]; }
    printf("ok %llu %llu\n", (unsigned long long)all, (unsigned long long)bands);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "constants")) {
        printf("%u %u %u %u %u %u\n", PLF_LANES, PLF_WAVES, PLF_BAND, PLF_K, PLF_LAG, PLF_RING);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "run")) return run_cases(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "sched")) return check_schedules((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]));
    if (argc >= 2 && !strcmp(argv[1], "barriers")) {
        for (int a = 2; a + 1 < argc; a += 2)
            printf("%llu\n", (unsigned long long)plf_barriers((uint32_t)strtoul(argv[a], nullptr, 10), (uint32_t)strtoul(argv[a + 1], nullptr, 10)));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "layout")) {
        std::vector<uint32_t> w;
        for (int a = 4; a < argc; a++) w.push_back((uint32_t)strtoul(argv[a], nullptr, 10));
        const size_t base = strtoull(argv[2], nullptr, 10), job_bytes = strtoull(argv[3], nullptr, 10);
        const PlDitherLayout l = pl_dither_layout(w, base, job_bytes);
        printf("jobs %zu %zu\n", l.jobs, job_bytes * (w.empty() ? 1 : w.size()));
        printf("lines %zu %zu\n", l.lines, l.lines_bytes);
        for (size_t i = 0; i < w.size(); i++) printf("line%zu %zu %zu\n", i, l.line[i], PLF_ERR_BYTES * (size_t)w[i]);
        printf("total 0 %zu\n", l.total);
        return 0;
    }
    return 2;
}

/* tests/c/quant_space_host.cpp -- test infrastructure: the quantiser in the premultiplied space (include/pngloss_hip_quant_space.h) run on the CPU
 * the way pl_quant.hip, pl_dither.hip and pl_host_quant.hip run it, under the sanitizers: the Visible bodies of pl_quant_core.h, pl_quant_measure_core.h
 * and pl_dither_core.h.  As in tests/c/quant_host.cpp, host threads stand in for the lanes of several workgroups (kGroup threads share one set of
 * 32-bit cells) and accumulate concurrently; as in tests/c/dither_host.cpp, the dither pass runs band by band, epoch by epoch, wave by wave, the waves
 * of an epoch ascending or descending, over rings and an error line that start out poisoned.
 * usage: quant_space_host straight out.bin        65 536 u32: plq_straight of the entry (c', c', c', a) at index a * 256 + c'
 *        quant_space_host run cases.bin out.bin
 *          cases.bin: u32 n; per case u32 width, height, max_colors, rounds, dither, threads, descending; width * height u32 words
 *          out.bin:   per case u32 entries (0: exact); entries words of the median cut's palette; entries words of the palette behind the rounds;
 *                     width * height u32 words: the image as it is now; 10 u64 as 20 u32: what the measuring lanes make of (input, final palette)
 *                     -- visible pixels, changed pixels, sq_err[4], max_abs[4] -- all zero for an exact or a dithered case */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "../../pngloss_amd/csrc/pl_layout.h"
#include "../../pngloss_amd/csrc/pl_quant_measure_core.h"
#include "../../pngloss_amd/csrc/pl_dither_core.h"

namespace {

constexpr uint32_t kGroup = 4;
constexpr uint32_t kCells = PLQ_MAX_COLORS * PLQ_CELLS;
constexpr uint32_t kPoison = 0x7FFF7FFFu;

void run_team(uint32_t threads, const std::function<void(uint32_t)> &fn)
{
    if (threads <= 1) { fn(0); return; }
    std::vector<std::thread> team;
    for (uint32_t t = 0; t < threads; t++) team.emplace_back(fn, t);
    for (auto &th : team) th.join();
}

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

void for_each_quad(uint32_t threads, size_t n, const std::function<void(uint32_t, size_t, uint32_t)> &fn)
{
    const size_t quads = (n + PLQ_QUAD - 1) / PLQ_QUAD;
    run_team(threads, [&](uint32_t t) {
        for (size_t q = t; q < quads; q += threads) {
            const size_t base = q * PLQ_QUAD;
            fn(t, base, n - base < PLQ_QUAD ? (uint32_t)(n - base) : PLQ_QUAD);
        }
    });
}

/* the tables a kernel of the premultiplied space builds at its start: plq_search's, and the straight word of every entry */
void load_tables(std::vector<uint32_t> &pal2, std::vector<uint32_t> &straight, const uint32_t *pal, uint32_t entries)
{
    pal2.assign(2 * PLQ_MAX_COLORS, 0);
    straight.assign(PLQ_MAX_COLORS, kPoison);
    for (uint32_t e = 0; e < entries; e++) { pal2[2 * e] = pal[e]; pal2[2 * e + 1] = plq_base(pal[e], e); straight[e] = plq_straight(pal[e]); }
}

/* what a lane does behind its load */
void space_quad(const uint32_t *p, uint32_t m, uint32_t *w)
{
    for (uint32_t k = 0; k < PLQ_QUAD; k++) w[k] = k < m ? p[k] : 0u;
    plq_space_quad<true>(w, m);
}

/* pl_dither_visible's body for one image (tests/c/dither_host.cpp: run_image, with the Visible step) */
bool dither_image(const uint32_t *img, uint32_t *out, uint32_t W, uint32_t H, const uint32_t *pal, uint32_t entries, bool descending)
{
    bool ok = true;
    std::vector<uint32_t> pal2, straight;
    load_tables(pal2, straight, pal, entries);
    const PlfErr zero = { 0u, 0u }, poison = { kPoison, kPoison };
    std::vector<PlfErr> ring(PLF_RING_ENTRIES, poison), line(W ? W : 1, poison);
    const uint64_t wave_epochs = plf_wave_epochs(W);
    const uint32_t bands = plf_bands(H);
    for (uint32_t band = 0; band < bands; band++) {
        const uint32_t rows = plf_band_rows(H, band), waves = plf_band_waves(rows);
        const uint64_t epochs = plf_band_epochs(W, waves);
        std::vector<PlfLane> lanes((size_t)PLF_WAVES * PLF_LANES, PlfLane{ zero, zero, zero, zero });
        for (uint64_t g = 0; g < epochs; g++) {
            for (uint32_t turn = 0; turn < PLF_WAVES; turn++) {
                const uint32_t wave = descending ? PLF_WAVES - 1 - turn : turn;
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
                    PlfErr fetch[PLF_LANES];
                    for (uint32_t lane = 0; lane < PLF_LANES; lane++) fetch[lane] = lane ? s[lane - 1].last : above(t + 1);
                    for (uint32_t lane = 0; lane < PLF_LANES; lane++) {
                        const int64_t x = plf_column(t, lane);
                        const uint32_t row = wave * PLF_LANES + lane;
                        plf_lane_shift(s[lane], fetch[lane]);
                        if (row < rows && x >= 0 && (uint64_t)x < W) {
                            const size_t at = ((size_t)band * PLF_BAND + row) * W + (size_t)x;
                            if (out[at] != kPoison) ok = false;             /* (visited twice) */
                            out[at] = plf_pixel<true>(pal2.data(), entries, img[at], s[lane].last, s[lane].ul, s[lane].up, s[lane].ur, &s[lane].last, nullptr, straight.data());
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
    return ok;
}

int run_cases(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!read_u32(in, &ncases, 1)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t head[7];
        if (!read_u32(in, head, 7)) return 3;
        const uint32_t W = head[0], H = head[1], N = head[2], R = head[3], threads = head[5] ? head[5] : 1;
        const bool dither = head[4] != 0, descending = head[6] != 0;
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> img(n ? n : 1);
        if (n && !read_u32(in, img.data(), n)) return 3;

        /* pl_index_count on the straight words, pl_quant_hist_visible */
        std::vector<uint64_t> table(PLI_SLOTS, PLI_EMPTY);
        uint32_t count = 0;
        const uint32_t groups = (threads + kGroup - 1) / kGroup;
        std::vector<uint64_t> cache((size_t)groups * PLI_CACHE, PLI_EMPTY);
        std::vector<uint32_t> hist(PLQ_BINS, 0), held0(threads, 0);   /* a lane's own count of bin 0 */
        for_each_quad(threads, n, [&](uint32_t t, size_t base, uint32_t m) {
            if (PLI_LOAD32(&count) <= PLI_MAX_COLORS)
                pli_count_quad(table.data(), &count, cache.data() + (size_t)(t / kGroup) * PLI_CACHE, img.data() + base, m, base != 0, base ? img[base - 1] : 0u);
            plq_hist_quad<true>(hist.data(), img.data() + base, m, &held0[t]);
        });
        for (uint32_t v : held0) if (v) PLQ_ADD32(hist.data(), v);      /* (the kernel: once per wave) */

        std::vector<uint32_t> first, pal;
        uint64_t record[10] = {};
        if (pli_colors_of(count) > N) {
            first = plq_median_cut(hist.data(), N);
            if (first.empty() || first.size() > N) return 4;
            const uint32_t entries = (uint32_t)first.size();
            pal = first;
            pal.resize(PLQ_MAX_COLORS, 0);
            std::vector<uint64_t> acc(kCells, 0);
            std::vector<uint32_t> pal2, straight, out_img(n, kPoison);
            for (uint32_t round = 0; round < R; round++) {
                /* pl_quant_assign_visible, pl_quant_update */
                load_tables(pal2, straight, pal.data(), entries);
                std::vector<uint32_t> cells((size_t)groups * kCells, 0);
                for_each_quad(threads, n, [&](uint32_t t, size_t base, uint32_t m) {
                    uint32_t w[PLQ_QUAD], best[PLQ_QUAD];
                    space_quad(img.data() + base, m, w);
                    plq_search_quad(pal2.data(), entries, w, m, best);
                    plq_accumulate_quad(cells.data() + (size_t)(t / kGroup) * kCells, w, best, m);
                });
                run_team(threads, [&](uint32_t t) {
                    const uint32_t lane = t % kGroup, lanes = std::min(kGroup, threads - t / kGroup * kGroup);
                    for (uint32_t i = lane; i < kCells; i += lanes) plq_flush_cell(acc.data(), cells.data() + (size_t)(t / kGroup) * kCells, i);
                });
                run_team(threads, [&](uint32_t t) { for (uint32_t k = t; k < PLQ_MAX_COLORS; k += threads) plq_update_entry(pal.data(), acc.data(), k); });
                for (uint64_t v : acc) if (v) return 5;
            }
            load_tables(pal2, straight, pal.data(), entries);
            if (dither) {
                if (!dither_image(img.data(), out_img.data(), W, H, pal.data(), entries, descending)) { fprintf(stderr, "case %u: a pixel visited twice\n", c); return 7; }
            } else {
                /* pl_quant_measure_visible: two workgroups of `threads` lanes; then pl_quant_remap_visible */
                PldSum total = {};
                for (uint32_t b = 0; b < 2; b++)
                    for (uint32_t l = 0; l < threads; l++) pld_merge(total, plq_measure_lane<true>(pal2.data(), entries, img.data(), n, b, 2, l, threads));
                record[0] = total.visible; record[1] = total.changed;
                for (int k = 0; k < 4; k++) { record[2 + k] = total.sq[k]; record[6 + k] = total.mx[k]; }
                for_each_quad(threads, n, [&](uint32_t, size_t base, uint32_t m) {
                    uint32_t w[PLQ_QUAD], best[PLQ_QUAD];
                    space_quad(img.data() + base, m, w);
                    plq_search_quad(pal2.data(), entries, w, m, best);
                    for (uint32_t k = 0; k < m; k++) out_img[base + k] = straight[best[k]];
                });
            }
            img = out_img;
        }
        const uint32_t entries = (uint32_t)first.size();
        fwrite(&entries, sizeof entries, 1, out);
        if (entries) {
            fwrite(first.data(), sizeof(uint32_t), entries, out);
            fwrite(pal.data(), sizeof(uint32_t), entries, out);
        }
        fwrite(img.data(), sizeof(uint32_t), n, out);
        fwrite(record, sizeof record, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 6;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "run")) return run_cases(argv[2], argv[3]);
    if (argc >= 3 && !strcmp(argv[1], "straight")) {
        std::vector<uint32_t> words(65536);
        for (uint32_t a = 0; a < 256; a++)
            for (uint32_t c = 0; c < 256; c++) words[a * 256 + c] = plq_straight(c | c << 8 | c << 16 | a << 24);
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(words.data(), sizeof(uint32_t), words.size(), f) != words.size()) return 3;
        return fclose(f) == 0 ? 0 : 6;
    }
    return 2;
}

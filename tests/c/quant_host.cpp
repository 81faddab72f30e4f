/* tests/c/quant_host.cpp -- test infrastructure: the bodies of pngloss_amd/csrc/pl_quant_core.h (histogram, search, accumulate, flush, update, the
 * host's median cut) run on the CPU the way pl_quant.hip and pl_host_quant.hip run them, under the sanitizers.  With one thread the lanes of a kernel
 * run one after the other; with a team, host threads stand in for the lanes of several workgroups (kGroup threads share one set of 32-bit cells, like
 * a workgroup's LDS) and accumulate concurrently.  The phases are separated by joins, as the kernels are by their launches.
 * usage: quant_host run cases.bin out.bin
 *          cases.bin: u32 n; per case u32 width, height, max_colors, rounds, threads; width * height u32 words
 *          out.bin:   per case u32 entries (0: exact); entries words of the median cut's palette; entries words of the palette behind the rounds;
 *                     u32 non-empty bins, u32 sum of the histogram; width * height u32 words: the image as it is now
 *        quant_host cut hist.bin max_colors       (65 536 u32 counts) prints the median cut's palette, one hex word per line
 *        quant_host grid pixels want ...          prints "pixels want blocks wg_pixels" per pair
 *        quant_host pixels width height ...      prints "width height pixels ok" per pair (plq_pixels_ok), then "limit PLQ_MAX_PIXELS"
 *        quant_host layout inputs w h [w h ...]   prints "name offset bytes" per region of pl_quant_layout, then "total 0 bytes" */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "../../pngloss_amd/csrc/pl_layout.h"

namespace {

constexpr uint32_t kGroup = 4;
constexpr uint32_t kCells = PLQ_MAX_COLORS * PLQ_CELLS;

/* fn(t) for t = 0 .. threads - 1: in turn with one thread, concurrently with a team */
void run_team(uint32_t threads, const std::function<void(uint32_t)> &fn)
{
    if (threads <= 1) { fn(0); return; }
    std::vector<std::thread> team;
    for (uint32_t t = 0; t < threads; t++) team.emplace_back(fn, t);
    for (auto &th : team) th.join();
}

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

/* fn(t, base, m) for every quad of n pixels, quad q on thread q % threads */
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

void load_pal2(std::vector<uint32_t> &pal2, const std::vector<uint32_t> &pal)
{
    pal2.assign(2 * PLQ_MAX_COLORS, 0);
    for (uint32_t e = 0; e < pal.size(); e++) { pal2[2 * e] = pal[e]; pal2[2 * e + 1] = plq_base(pal[e], e); }
}

int run_cases(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!read_u32(in, &ncases, 1)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t head[5];
        if (!read_u32(in, head, 5)) return 3;
        const uint32_t W = head[0], H = head[1], N = head[2], R = head[3], threads = head[4] ? head[4] : 1;
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> img(n ? n : 1);
        if (n && !read_u32(in, img.data(), n)) return 3;

        /* pl_index_count and pl_quant_hist */
        std::vector<uint64_t> table(PLI_SLOTS, PLI_EMPTY);
        uint32_t count = 0;
        const uint32_t groups = (threads + kGroup - 1) / kGroup;
        std::vector<uint64_t> cache((size_t)groups * PLI_CACHE, PLI_EMPTY);
        std::vector<uint32_t> hist(PLQ_BINS, 0);
        for_each_quad(threads, n, [&](uint32_t t, size_t base, uint32_t m) {
            if (PLI_LOAD32(&count) <= PLI_MAX_COLORS)
                pli_count_quad(table.data(), &count, cache.data() + (size_t)(t / kGroup) * PLI_CACHE, img.data() + base, m, base != 0, base ? img[base - 1] : 0u);
            plq_hist_quad(hist.data(), img.data() + base, m);
        });
        uint32_t nonzero = 0, sum = 0;
        for (uint32_t v : hist) { nonzero += v ? 1u : 0u; sum += v; }

        std::vector<uint32_t> first, pal;
        if (pli_colors_of(count) > N) {
            first = plq_median_cut(hist.data(), N);
            if (first.empty() || first.size() > N) return 4;
            pal = first;
            pal.resize(PLQ_MAX_COLORS, 0);
            std::vector<uint64_t> acc(kCells, 0);
            std::vector<uint32_t> pal2, out_img(n);
            for (uint32_t round = 0; round < R; round++) {
                /* pl_quant_assign: search, accumulate in the group's cells; then -- behind the barrier -- every cell flushed by one thread of its group */
                load_pal2(pal2, std::vector<uint32_t>(pal.begin(), pal.begin() + (long)first.size()));
                std::vector<uint32_t> cells((size_t)groups * kCells, 0);
                for_each_quad(threads, n, [&](uint32_t t, size_t base, uint32_t m) {
                    uint32_t best[PLQ_QUAD];
                    plq_search_quad(pal2.data(), (uint32_t)first.size(), img.data() + base, m, best);
                    plq_accumulate_quad(cells.data() + (size_t)(t / kGroup) * kCells, img.data() + base, best, m);
                });
                run_team(threads, [&](uint32_t t) {
                    const uint32_t lane = t % kGroup, lanes = std::min(kGroup, threads - t / kGroup * kGroup);
                    for (uint32_t i = lane; i < kCells; i += lanes) plq_flush_cell(acc.data(), cells.data() + (size_t)(t / kGroup) * kCells, i);
                });
                /* pl_quant_update */
                run_team(threads, [&](uint32_t t) { for (uint32_t k = t; k < PLQ_MAX_COLORS; k += threads) plq_update_entry(pal.data(), acc.data(), k); });
                for (uint64_t v : acc) if (v) return 5;
            }
            /* pl_quant_remap, then the copy over the input */
            load_pal2(pal2, std::vector<uint32_t>(pal.begin(), pal.begin() + (long)first.size()));
            for_each_quad(threads, n, [&](uint32_t, size_t base, uint32_t m) {
                uint32_t best[PLQ_QUAD];
                plq_search_quad(pal2.data(), (uint32_t)first.size(), img.data() + base, m, best);
                for (uint32_t k = 0; k < m; k++) out_img[base + k] = pal2[2 * best[k]];
            });
            img = out_img;
        }
        const uint32_t entries = (uint32_t)first.size();
        fwrite(&entries, sizeof entries, 1, out);
        if (entries) {
            fwrite(first.data(), sizeof(uint32_t), entries, out);
            fwrite(pal.data(), sizeof(uint32_t), entries, out);
        }
        const uint32_t tail[2] = { nonzero, sum };
        fwrite(tail, sizeof tail, 1, out);
        fwrite(img.data(), sizeof(uint32_t), n, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 6;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "run")) return run_cases(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "cut")) {
        std::vector<uint32_t> hist(PLQ_BINS);
        FILE *f = fopen(argv[2], "rb");
        if (!f || !read_u32(f, hist.data(), PLQ_BINS)) return 3;
        fclose(f);
        for (uint32_t word : plq_median_cut(hist.data(), (uint32_t)atoi(argv[3]))) printf("%08x\n", word);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "grid")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const uint64_t pixels = strtoull(argv[a], nullptr, 10);
            const uint32_t want = (uint32_t)strtoul(argv[a + 1], nullptr, 10), blocks = plq_blocks(pixels, 256 * PLQ_QUAD, want);
            printf("%llu %u %u %llu\n", (unsigned long long)pixels, want, blocks, (unsigned long long)plq_wg_pixels(pixels, 256 * PLQ_QUAD, blocks));
        }
        printf("limits %llu %u %llu\n", (unsigned long long)PLQ_WG_PIXELS, PLQ_MAX_BLOCKS, (unsigned long long)PLQ_MAX_PIXELS);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "pixels")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const uint32_t w = (uint32_t)strtoul(argv[a], nullptr, 10), h = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
            const uint64_t px = (uint64_t)w * h;                    /* (the product as the argument check takes it) */
            printf("%u %u %llu %d\n", w, h, (unsigned long long)px, plq_pixels_ok(px) ? 1 : 0);
        }
        printf("limit %llu\n", (unsigned long long)PLQ_MAX_PIXELS);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "layout")) {
        std::vector<uint32_t> w, h;
        for (int a = 3; a + 1 < argc; a += 2) { w.push_back((uint32_t)atoi(argv[a])); h.push_back((uint32_t)atoi(argv[a + 1])); }
        const size_t jb[5] = { 64, 56, 32, sizeof(PliRecord), 64 };
        const PlQuantLayout l = pl_quant_layout(w, h, atoi(argv[2]) != 0, jb[0], jb[1], jb[2], jb[3], jb[4]);
        const size_t n = w.size(), n1 = n ? n : 1;
        auto put = [](const char *name, size_t i, size_t at, size_t bytes) { printf("%s%zu %zu %zu\n", name, i, at, bytes); };
        put("index_jobs", 0, l.index_jobs, jb[0] * n1); put("quant_jobs", 0, l.quant_jobs, jb[1] * n1); put("distort_jobs", 0, l.distort_jobs, jb[2] * n1);
        put("counts", 0, l.counts, 4 * n1); put("records", 0, l.records, jb[3] * n1); put("distort_records", 0, l.distort_records, jb[4] * n1);
        put("zeroed", 0, l.counts, l.zeroed); put("tables", 0, l.tables, l.tables_bytes); put("hists", 0, l.hists, l.hists_bytes);
        put("pals", 0, l.pals, PLL_QUANT_PAL * n1);
        for (size_t i = 0; i < n; i++) {
            const size_t bytes = (size_t)w[i] * h[i] * 4;
            put("table", i, l.im[i].table, sizeof(uint64_t) * PLI_SLOTS); put("hist", i, l.im[i].hist, PLL_QUANT_HIST); put("pal", i, l.im[i].pal, PLL_QUANT_PAL);
            put("acc", i, l.im[i].acc, PLL_QUANT_ACC); put("out", i, l.im[i].out, bytes); put("in", i, l.im[i].in, atoi(argv[2]) ? bytes : 0);
        }
        put("total", 0, 0, l.total);
        return 0;
    }
    return 2;
}

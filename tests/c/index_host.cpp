/* tests/c/index_host.cpp -- test infrastructure: the bodies of pngloss_amd/csrc/pl_index_core.h (insert, count, collect, rank, assign, lookup,
 * pack) run on the CPU the way pl_index.hip runs them, under the sanitizers.  With one thread the lanes of a kernel run one after the other;
 * with a team, host threads stand in for the lanes of several workgroups (kGroup threads share one pre-filter, like a workgroup's LDS) and insert
 * into the same table concurrently.  The phases are separated by joins, as the kernels are by their launches.
 * usage: index_host cases.bin out.bin
 *   cases.bin: u32 n; per case u32 width, height, threads; width * height u32 words
 *   out.bin:   per case u32 count, entries (0: not eligible), trns_entries, pitch; if entries: entries u32 words, height ids, height * pitch rows */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#include "../../pngloss_amd/csrc/pl_layout.h"

namespace {

constexpr uint32_t kGroup = 4;

/* fn(t) for t = 0 .. threads - 1: in turn with one thread, concurrently with a team */
void run_team(uint32_t threads, const std::function<void(uint32_t)> &fn)
{
    if (threads <= 1) { fn(0); return; }
    std::vector<std::thread> team;
    for (uint32_t t = 0; t < threads; t++) team.emplace_back(fn, t);
    for (auto &th : team) th.join();
}

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!read_u32(in, &ncases, 1)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t head[3];
        if (!read_u32(in, head, 3)) return 3;
        const uint32_t W = head[0], H = head[1], threads = head[2] ? head[2] : 1;
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> img(n ? n : 1);
        if (n && !read_u32(in, img.data(), n)) return 3;

        /* the layout the library uses for a one-image window: the pitch of the rows comes from there */
        const PlIndexLayout lay = pl_index_layout({ W }, { H }, 64, sizeof(PliRecord));
        const uint32_t pitch = lay.im[0].pitch;
        if (n && (pitch % 16 || pitch < W)) return 4;

        std::vector<uint64_t> table(PLI_SLOTS, PLI_EMPTY);
        uint32_t count = 0;
        const uint32_t groups = (threads + kGroup - 1) / kGroup;
        std::vector<uint64_t> cache((size_t)groups * PLI_CACHE, PLI_EMPTY);
        const size_t quads = (n + PLI_QUAD - 1) / PLI_QUAD;
        /* pl_index_count: a lane leaves once the counter is past 256, else takes its next quad */
        run_team(threads, [&](uint32_t t) {
            for (size_t q = t; q < quads; q += threads) {
                if (PLI_LOAD32(&count) > PLI_MAX_COLORS) return;
                const size_t base = q * PLI_QUAD;
                const uint32_t m = n - base < PLI_QUAD ? (uint32_t)(n - base) : PLI_QUAD;
                pli_count_quad(table.data(), &count, cache.data() + (size_t)(t / kGroup) * PLI_CACHE, img.data() + base, m, base != 0, base ? img[base - 1] : 0u);
            }
        });

        uint32_t headout[4] = { count, 0, 0, pitch };
        if (count < 1 || count > PLI_MAX_COLORS) { fwrite(headout, sizeof headout, 1, out); continue; }

        /* pl_index_palette */
        PliRecord rec{};
        std::vector<uint32_t> list_word(PLI_MAX_COLORS), list_slot(PLI_MAX_COLORS);
        uint32_t m = 0;
        run_team(threads, [&](uint32_t t) { for (uint32_t s = t; s < PLI_SLOTS; s += threads) pli_collect(table.data(), s, list_word.data(), list_slot.data(), &m); });
        const uint32_t entries = std::min(m, PLI_MAX_COLORS);
        run_team(threads, [&](uint32_t t) { for (uint32_t k = t; k < entries; k += threads) pli_assign(table.data(), list_word.data(), list_slot.data(), entries, k, &rec); });
        rec.entries = m;

        /* pl_index_rows: whole dwords, the tail's unused bytes 0; the bytes between width rounded up to 4 and the pitch are never written */
        std::vector<uint8_t> rows((size_t)pitch * H, 0xEE), ids(H, 0xEE);
        const uint32_t row_quads = (W + PLI_QUAD - 1) / PLI_QUAD;
        run_team(threads, [&](uint32_t t) {
            for (size_t q = t; q < (size_t)row_quads * H; q += threads) {
                const uint32_t y = (uint32_t)(q / row_quads), x = (uint32_t)(q % row_quads) * PLI_QUAD, mm = W - x < PLI_QUAD ? W - x : PLI_QUAD;
                if (x == 0) ids[y] = 0;
                const uint32_t v = pli_pack_quad(table.data(), img.data() + (size_t)y * W + x, mm);
                uint8_t *d = rows.data() + (size_t)y * pitch + x;
                for (int b = 0; b < 4; b++) d[b] = (uint8_t)(v >> (8 * b));
            }
        });

        headout[1] = rec.entries; headout[2] = rec.trns_entries;
        fwrite(headout, sizeof headout, 1, out);
        fwrite(rec.words, sizeof(uint32_t), rec.entries, out);
        fwrite(ids.data(), 1, H, out);
        fwrite(rows.data(), 1, rows.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 5;
}

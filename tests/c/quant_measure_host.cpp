/* tests/c/quant_measure_host.cpp -- test infrastructure: the lane loop of pl_quant_measure (pngloss_amd/csrc/pl_quant_measure_core.h) run on the CPU
 * the way pl_quant.hip runs it, under the sanitizers.  `blocks` workgroups of `lanes` lanes walk the image; with team = 0 the lanes run one after the
 * other, with team = 1 every lane is a host thread and the sums are merged concurrently, with the atomics the kernel leaves in the record.
 * usage: quant_measure_host run cases.bin out.bin
 *          cases.bin: u32 n; per case u32 width, height, entries, blocks, lanes, team, offset_words; `entries` palette words; width * height words
 *                     (the image is copied to a heap block that starts offset_words words behind a 16-byte boundary and ends with its last word,
 *                     so that a load past either end is a report)
 *          out.bin:   per case u64 changed_pixels, sq_err[4], max_abs[4]
 *        quant_measure_host constants     prints PLD_FLUSH_PIXELS PLD_LANE_PIXELS_MAX PLQ_WG_PIXELS PLQ_QUAD */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../pngloss_amd/csrc/pl_quant_measure_core.h"

namespace {

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

void merge(PlDistortRecord &r, const PldSum &s)
{
    for (int c = 0; c < 4; c++) {
        if (s.sq[c]) PLQ_ADD64(&r.sq_err[c], s.sq[c]);
        uint32_t seen = __atomic_load_n(&r.max_abs[c], __ATOMIC_RELAXED);
        while (s.mx[c] > seen && !__atomic_compare_exchange_n(&r.max_abs[c], &seen, s.mx[c], false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    if (s.changed) PLQ_ADD64(&r.changed_pixels, s.changed);
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
        const uint32_t W = head[0], H = head[1], entries = head[2], blocks = head[3], lanes = head[4], team = head[5], offset = head[6];
        if (!entries || entries > PLQ_MAX_COLORS || !blocks || !lanes || offset >= 4) return 2;
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> pal(entries), pal2(2 * PLQ_MAX_COLORS, 0);
        if (!read_u32(in, pal.data(), entries)) return 3;
        for (uint32_t e = 0; e < entries; e++) { pal2[2 * e] = pal[e]; pal2[2 * e + 1] = plq_base(pal[e], e); }
        void *block = nullptr;
        const size_t bytes = (n + offset) * sizeof(uint32_t);
        if (posix_memalign(&block, 16, bytes > 0 ? bytes : 1)) return 2;
        uint32_t *img = static_cast<uint32_t *>(block) + offset;
        if (n && !read_u32(in, img, n)) return 3;

        PlDistortRecord rec = {};
        auto lane = [&](uint32_t b, uint32_t l) { merge(rec, plq_measure_lane(pal2.data(), entries, img, n, b, blocks, l, lanes)); };
        if (team) {
            std::vector<std::thread> threads;
            for (uint32_t b = 0; b < blocks; b++)
                for (uint32_t l = 0; l < lanes; l++) threads.emplace_back(lane, b, l);
            for (auto &t : threads) t.join();
        } else {
            for (uint32_t b = 0; b < blocks; b++)
                for (uint32_t l = 0; l < lanes; l++) lane(b, l);
        }
        std::free(block);
        const uint64_t words[9] = { rec.changed_pixels, rec.sq_err[0], rec.sq_err[1], rec.sq_err[2], rec.sq_err[3], rec.max_abs[0], rec.max_abs[1], rec.max_abs[2], rec.max_abs[3] };
        fwrite(words, sizeof words, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 6;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "run")) return run_cases(argv[2], argv[3]);
    if (argc >= 2 && !strcmp(argv[1], "constants")) {
        printf("%u %u %llu %u\n", PLD_FLUSH_PIXELS, PLD_LANE_PIXELS_MAX, (unsigned long long)PLQ_WG_PIXELS, PLQ_QUAD);
        return 0;
    }
    return 2;
}

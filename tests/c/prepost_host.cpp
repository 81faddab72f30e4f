/*
 * prepost_host.cpp -- TEST INFRASTRUCTURE: the rules of the kernels around the row engine (pngloss_amd/csrc/pl_prepost_core.h, shared with
 * pl_prepost.hip) on the CPU.  Built with -fsanitize=address,undefined and run by tests/test_prepost_host.py, which compares everything it prints
 * with the oracle and with numpy / Python restatements (tests/util_prepost.py).  Never shipped.
 *
 *   prepost_host CASES
 * CASES: uint64 count, then per case uint64 { width, height, bpp, offset, blocks, threads } and width * height pixel words ("slots" layout: channel c in
 * byte c, bpp channels used).  The image gets a heap block of its own that starts `offset` bytes behind a 16-byte boundary and ends with its last
 * pixel, so a load outside the image is a report.  pl_hist's thread loop (plp_hist_thread) runs in the kernel's order -- workgroup 0 .. blocks - 1,
 * thread 0 .. threads - 1, each through all its trips -- over ONE table; every pixel adds the five bins of each of its bpp channels (plp_bins).
 * Prints per case two lines: the 5 * 256 counts, then their 5 * 256 ranks (plp_rank), and on a third which loader ran and how many pixels were counted.
 *
 *   prepost_host bytes OUT
 * pl_sub4 and pl_avg4 over all 65 536 byte pairs (a, b) in each of the four byte lanes, the other three lanes of a and of b at 0x00 or 0xff (the four
 * combinations): writes to OUT, per (lane, fill of a, fill of b, a, b) in that nesting, the two result words.
 *
 *   prepost_host loader W ADDRESS N [W ADDRESS N ...]          plp_quad_loader per triple (the address is never read)
 *   prepost_host quad Q W4 [...]                               plp_quad_at: has_up has_left up left diag
 *   prepost_host pixel I W [...]                               plp_pixel_at: has_up has_left up left diag
 *   prepost_host rank FILE                                     FILE: uint64 count, then count tables of 256 uint32; prints per table its 256 ranks
 *   prepost_host grid batch N MAX_PX PX_PER_THREAD | hist N MAX_PX NT CAP | slice N FIRST [...]
 * prints PLP_MAX_IMAGES and PLP_THREADS on one line, then per item plp_batch_blocks / plp_hist_blocks / plp_slice.
 */
#include "../../pngloss_amd/csrc/pl_prepost_core.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t num(const char *s) { return std::strtoull(s, nullptr, 0); }

struct Table {
    uint32_t n[PLP_NFILT][PLP_NSYM];
    uint64_t pixels;
    int bpp;
    void operator()(uint32_t here, uint32_t left, uint32_t above, uint32_t diag)
    {
        const PlpResidual r = plp_residual(here, left, above);
        for (int c = 0; c < bpp; c++) {
            uint32_t bin[PLP_NFILT];
            plp_bins(bin, c, here, left, above, diag, r);
            for (int f = 0; f < PLP_NFILT; f++) {
                if (bin[f] >= (uint32_t)PLP_NSYM) std::abort();
                n[f][bin[f]]++;
            }
        }
        pixels++;
    }
};

static int cases(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t head[6];
        if (std::fread(head, 8, 6, f) != 6) return 2;
        const uint64_t W = head[0], H = head[1], bpp = head[2], offset = head[3], blocks = head[4], threads = head[5];
        if (bpp < 1 || bpp > 4 || offset % 4 || !blocks || !threads || W > 0xffffffffu || H > 0xffffffffu) return 2;
        const size_t n = (size_t)(W * H);
        void *base = nullptr;
        if (posix_memalign(&base, 16, n * 4 + offset + (n * 4 + offset == 0)) != 0) return 2;
        uint32_t *img = reinterpret_cast<uint32_t *>(static_cast<char *>(base) + offset);
        if (n && std::fread(img, 4, n, f) != n) return 2;
        static Table t;
        std::memset(&t, 0, sizeof t);
        t.bpp = (int)bpp;
        for (uint64_t b = 0; b < blocks; b++)
            for (uint64_t th = 0; th < threads; th++) plp_hist_thread(img, (uint32_t)W, n, (uint32_t)b, (uint32_t)th, (uint32_t)blocks, (uint32_t)threads, t);
        for (int fi = 0; fi < PLP_NFILT; fi++)
            for (int s = 0; s < PLP_NSYM; s++) std::printf("%u ", t.n[fi][s]);
        std::printf("\n");
        for (int fi = 0; fi < PLP_NFILT; fi++)
            for (int s = 0; s < PLP_NSYM; s++) std::printf("%u ", plp_rank(t.n[fi], t.n[fi][s]));
        std::printf("\n%d %" PRIu64 "\n", plp_quad_loader((uint32_t)W, img, n) ? 1 : 0, t.pixels);
        std::free(base);
    }
    std::fclose(f);
    return 0;
}

static int bytes(const char *path)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return 2;
    std::vector<uint32_t> out;
    out.reserve(4 * 4 * 65536 * 2);
    for (int lane = 0; lane < 4; lane++)
        for (int fa = 0; fa < 2; fa++)
            for (int fb = 0; fb < 2; fb++) {
                const uint32_t keep = ~(0xffu << (8 * lane));
                const uint32_t wa = (fa ? 0xffffffffu : 0u) & keep, wb = (fb ? 0xffffffffu : 0u) & keep;
                for (uint32_t a = 0; a < 256; a++)
                    for (uint32_t b = 0; b < 256; b++) {
                        out.push_back(pl_sub4(wa | (a << (8 * lane)), wb | (b << (8 * lane))));
                        out.push_back(pl_avg4(wa | (a << (8 * lane)), wb | (b << (8 * lane))));
                    }
            }
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

static int rank(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint32_t h[PLP_NSYM];
        if (std::fread(h, 4, PLP_NSYM, f) != (size_t)PLP_NSYM) return 2;
        for (int s = 0; s < PLP_NSYM; s++) std::printf("%u ", plp_rank(h, h[s]));
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}

static int grid(int argc, char **argv)
{
    std::printf("%zu %u\n", PLP_MAX_IMAGES, PLP_THREADS);
    for (int k = 2; k < argc;) {
        if (std::strcmp(argv[k], "batch") == 0 && k + 3 < argc) {
            if (!num(argv[k + 1])) return 2;
            std::printf("%zu\n", plp_batch_blocks((size_t)num(argv[k + 1]), (size_t)num(argv[k + 2]), (uint32_t)num(argv[k + 3])));
            k += 4;
        } else if (std::strcmp(argv[k], "hist") == 0 && k + 4 < argc) {
            if (!num(argv[k + 1])) return 2;
            std::printf("%zu\n", plp_hist_blocks((size_t)num(argv[k + 1]), (size_t)num(argv[k + 2]), (uint32_t)num(argv[k + 3]), (unsigned)num(argv[k + 4])));
            k += 5;
        } else if (std::strcmp(argv[k], "slice") == 0 && k + 2 < argc) {
            if (num(argv[k + 2]) >= num(argv[k + 1])) return 2;
            std::printf("%zu\n", plp_slice((size_t)num(argv[k + 1]), (size_t)num(argv[k + 2])));
            k += 3;
        } else return 2;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (std::strcmp(argv[1], "bytes") == 0) return argc == 3 ? bytes(argv[2]) : 2;
    if (std::strcmp(argv[1], "rank") == 0) return argc == 3 ? rank(argv[2]) : 2;
    if (std::strcmp(argv[1], "grid") == 0) return grid(argc, argv);
    if (std::strcmp(argv[1], "loader") == 0) {
        if ((argc - 2) % 3) return 2;
        for (int k = 2; k < argc; k += 3)
            std::printf("%d\n", plp_quad_loader((uint32_t)num(argv[k]), reinterpret_cast<const void *>((uintptr_t)num(argv[k + 1])), (size_t)num(argv[k + 2])) ? 1 : 0);
        return 0;
    }
    if (std::strcmp(argv[1], "quad") == 0) {
        if ((argc - 2) % 2) return 2;
        for (int k = 2; k < argc; k += 2) {
            if (!num(argv[k + 1])) return 2;
            const PlpQuadAt a = plp_quad_at((uint32_t)num(argv[k]), (uint32_t)num(argv[k + 1]));
            std::printf("%d %d %u %zu %zu\n", a.has_up, a.has_left, a.up, a.left, a.diag);
        }
        return 0;
    }
    if (std::strcmp(argv[1], "pixel") == 0) {
        if ((argc - 2) % 2) return 2;
        for (int k = 2; k < argc; k += 2) {
            if (!num(argv[k + 1])) return 2;
            const PlpPixelAt a = plp_pixel_at((size_t)num(argv[k]), (uint32_t)num(argv[k + 1]));
            std::printf("%d %d %zu %zu %zu\n", a.has_up, a.has_left, a.up, a.left, a.diag);
        }
        return 0;
    }
    return argc == 2 ? cases(argv[1]) : 2;
}

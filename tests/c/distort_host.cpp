/*
 * distort_host.cpp -- TEST INFRASTRUCTURE: the arithmetic of the distortion measurement (pngloss_amd/csrc/pl_distort_core.h, shared with the HIP
 * kernel pl_distort) on the CPU: the kernel's thread loop run for tid = 0 .. nthreads - 1, the sums merged, the record printed.  Built with
 * -fsanitize=address,undefined and run by tests/test_distort_host.py, which compares every record with numpy.  Never shipped.
 *
 *   distort_host CASES
 * CASES: uint64 count, then per case uint64 { pixels, a_offset, b_offset, nthreads } and pixels words of a, pixels words of b.  Each image gets a heap
 * block of its own that starts a_offset / b_offset bytes behind a 16-byte boundary and ends with its last pixel, so a load past an image is a report.
 * Prints per case one line: pixels changed_pixels sq_err[0..3] max_abs[0..3].
 *
 *   distort_host grid N MAX_PIXELS [N MAX_PIXELS ...]
 * The launch shape of pl_distort.hip: prints PLD_MAX_IMAGES and PLD_THREADS on one line, then per (N, MAX_PIXELS) pld_grid_blocks(N, MAX_PIXELS); N >= 1.
 */
#include "../../pngloss_amd/csrc/pl_distort_core.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint32_t *block(FILE *f, uint64_t pixels, uint64_t offset, void **base)
{
    if (posix_memalign(base, 16, (size_t)(pixels * 4 + offset) + (pixels * 4 + offset == 0)) != 0) return nullptr;
    uint32_t *p = reinterpret_cast<uint32_t *>(static_cast<char *>(*base) + offset);
    if (pixels && std::fread(p, 4, (size_t)pixels, f) != (size_t)pixels) return nullptr;
    return p;
}

static int grid(int argc, char **argv)
{
    if (argc % 2) return 2;
    std::printf("%zu %u\n", PLD_MAX_IMAGES, PLD_THREADS);
    for (int k = 2; k < argc; k += 2) {
        const uint64_t n = std::strtoull(argv[k], nullptr, 10), max_pixels = std::strtoull(argv[k + 1], nullptr, 10);
        if (!n) return 2;
        std::printf("%zu\n", pld_grid_blocks((size_t)n, max_pixels));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::strcmp(argv[1], "grid") == 0) return grid(argc, argv);
    FILE *f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t head[4];
        if (std::fread(head, 8, 4, f) != 4 || head[1] % 4 || head[2] % 4 || !head[3]) return 2;
        void *base_a = nullptr, *base_b = nullptr;
        const uint32_t *a = block(f, head[0], head[1], &base_a), *b = block(f, head[0], head[2], &base_b);
        if (!a || !b) return 2;
        PldSum sum = {};
        for (uint64_t tid = 0; tid < head[3]; tid++) pld_merge(sum, pld_thread(a, b, (size_t)head[0], (size_t)tid, (size_t)head[3]));
        PlDistortRecord r;
        pld_record(r, sum, head[0]);
        std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u\n", r.pixels, r.changed_pixels, r.sq_err[0], r.sq_err[1], r.sq_err[2],
                    r.sq_err[3], r.max_abs[0], r.max_abs[1], r.max_abs[2], r.max_abs[3]);
        std::free(base_a);
        std::free(base_b);
    }
    std::fclose(f);
    return 0;
}

/*
 * visible_host.cpp -- TEST INFRASTRUCTURE: the visible mode of the two measurements (pngloss_amd/csrc/pl_distort_core.h and pl_ssim_core.h, shared
 * with the HIP kernels pl_distort_visible and pl_ssim_visible) on the CPU: the kernels' thread loops in their visible instantiation run for
 * tid = 0 .. nthreads - 1, the partial results merged, the records printed.  Built with -fsanitize=address,undefined and run by
 * tests/test_visible_host.py, which compares every record with numpy (tests/util_visible.py).  Never shipped, never loaded into Python.
 *
 *   visible_host pm            prints pm of the pixel (c, c, c, A) for A = 0 .. 255 (outer), c = 0 .. 255: one hexadecimal word per line, from
 *                              pld_pm; a disagreement of pls_pm is exit code 3
 *   visible_host CASES         CASES: uint64 count, then per case uint64 { kind, width, height, a_offset, b_offset, nthreads } and width * height
 *                              words of a, then of b.  kind 0: the distortion record (the image is width * height pixels in a row); kind 1: the
 *                              SSIM record (nthreads a multiple of 4).  Each image gets a heap block of its own that starts a_offset / b_offset
 *                              bytes behind a 16-byte boundary and ends with its last pixel, so a load past an image is a report.
 * Prints per case one line: kind 0: pixels changed_pixels sq_err[0..3] max_abs[0..3]; kind 1: windows sum_q16[0..3] min_q16[0..3] reserved.
 */
#include "../../pngloss_amd/csrc/pl_distort_core.h"
#include "../../pngloss_amd/csrc/pl_ssim_core.h"

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

static int all_pm()
{
    for (uint32_t A = 0; A < 256; A++)
        for (uint32_t c = 0; c < 256; c++) {
            const uint32_t p = c | c << 8 | c << 16 | A << 24;
            if (pld_pm(p) != pls_pm(p)) return 3;
            std::printf("%08x\n", pld_pm(p));
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "pm") == 0) return all_pm();
    FILE *f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t head[6];
        if (std::fread(head, 8, 6, f) != 6 || head[0] > 1 || head[3] % 4 || head[4] % 4 || !head[5] || (head[0] == 1 && head[5] % 4)) return 2;
        const uint32_t width = (uint32_t)head[1], height = (uint32_t)head[2], nthreads = (uint32_t)head[5];
        const uint64_t pixels = head[1] * head[2];
        void *base_a = nullptr, *base_b = nullptr, *base_t = nullptr;
        const uint32_t *a = block(f, pixels, head[3], &base_a), *b = block(f, pixels, head[4], &base_b);
        if (!a || !b) return 2;
        if (head[0] == 0) {
            PldSum sum = {};
            for (uint64_t tid = 0; tid < nthreads; tid++) pld_merge(sum, pld_thread<true>(a, b, (size_t)pixels, (size_t)tid, (size_t)nthreads));
            PlDistortRecord r;
            pld_record(r, sum, sum.visible);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u\n", r.pixels, r.changed_pixels, r.sq_err[0], r.sq_err[1],
                        r.sq_err[2], r.sq_err[3], r.max_abs[0], r.max_abs[1], r.max_abs[2], r.max_abs[3]);
        } else {
            if (posix_memalign(&base_t, 16, sizeof(PlsCell) * PLS_TILE_CELLS * 4) != 0) return 2;
            PlsCell *table = static_cast<PlsCell *>(base_t);
            const PlsGeom g = pls_geom(width, height);
            PlSsimRecord r = pls_record_begin_visible();
            for (uint64_t tile = 0; tile < g.tiles; tile++) {
                std::memset(table, 0xA5, sizeof(PlsCell) * PLS_TILE_CELLS * 4);      /* what a tile does not write, it must not read */
                for (uint32_t tid = 0; tid < nthreads; tid++) pls_thread_cells<true>(table, a, b, width, height, g, tile, tid, nthreads);
                for (uint32_t tid = 0; tid < nthreads; tid++) {
                    PlsPart p = pls_part();
                    pls_thread_windows<true>(p, table, g, tile, tid, nthreads);
                    if ((tid & 3) != 3 && p.windows) return 4;                       /* only the pairs of channel 3 count windows */
                    r.sum_q16[tid & 3] += p.sum;
                    if (p.mn < r.min_q16[tid & 3]) r.min_q16[tid & 3] = p.mn;
                    r.windows += p.windows;
                }
            }
            std::printf("%" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d %d %" PRIu64 "\n", r.windows, r.sum_q16[0], r.sum_q16[1], r.sum_q16[2],
                        r.sum_q16[3], r.min_q16[0], r.min_q16[1], r.min_q16[2], r.min_q16[3], r.reserved);
        }
        std::free(base_a);
        std::free(base_b);
        std::free(base_t);
    }
    std::fclose(f);
    return 0;
}

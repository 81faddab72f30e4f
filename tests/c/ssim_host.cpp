/*
 * ssim_host.cpp -- TEST INFRASTRUCTURE: the arithmetic of the SSIM measurement (pngloss_amd/csrc/pl_ssim_core.h, shared with the HIP kernel
 * pl_ssim) on the CPU: per tile the kernel's two thread loops run for tid = 0 .. nthreads - 1 over a table the size of the kernel's LDS one, the
 * partial records merged by channel, the record printed.  Built with -fsanitize=address,undefined and run by tests/test_ssim_host.py, which compares
 * every record with a restatement in Python integers.  Never shipped.
 *
 *   ssim_host CASES
 * CASES: uint64 count, then per case uint64 { width, height, a_offset, b_offset, nthreads } and width * height words of a, then of b.  Each image
 * gets a heap block of its own that starts a_offset / b_offset bytes behind a 16-byte boundary and ends with its last pixel, so a load past an
 * image is a report; the table is a heap block of exactly PLS_TILE_CELLS * 4 entries.
 * Prints per case one line: windows sum_q16[0..3] min_q16[0..3] reserved.
 */
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

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t head[5];
        if (std::fread(head, 8, 5, f) != 5 || head[2] % 4 || head[3] % 4 || !head[4] || head[4] % 4) return 2;
        const uint32_t width = (uint32_t)head[0], height = (uint32_t)head[1], nthreads = (uint32_t)head[4];
        void *base_a = nullptr, *base_b = nullptr, *base_t = nullptr;
        const uint32_t *a = block(f, head[0] * head[1], head[2], &base_a), *b = block(f, head[0] * head[1], head[3], &base_b);
        if (!a || !b || posix_memalign(&base_t, 16, sizeof(PlsCell) * PLS_TILE_CELLS * 4) != 0) return 2;
        PlsCell *table = static_cast<PlsCell *>(base_t);
        const PlsGeom g = pls_geom(width, height);
        PlSsimRecord r = pls_record_begin(width, height);
        for (uint64_t tile = 0; tile < g.tiles; tile++) {
            std::memset(table, 0xA5, sizeof(PlsCell) * PLS_TILE_CELLS * 4);      /* what a tile does not write, it must not read */
            for (uint32_t tid = 0; tid < nthreads; tid++) pls_thread_cells(table, a, b, width, height, g, tile, tid, nthreads);
            for (uint32_t tid = 0; tid < nthreads; tid++) {
                PlsPart p = pls_part();
                pls_thread_windows(p, table, g, tile, tid, nthreads);
                r.sum_q16[tid & 3] += p.sum;
                if (p.mn < r.min_q16[tid & 3]) r.min_q16[tid & 3] = p.mn;
            }
        }
        std::printf("%" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d %d %" PRIu64 "\n", r.windows, r.sum_q16[0], r.sum_q16[1], r.sum_q16[2],
                    r.sum_q16[3], r.min_q16[0], r.min_q16[1], r.min_q16[2], r.min_q16[3], r.reserved);
        std::free(base_a);
        std::free(base_b);
        std::free(base_t);
    }
    std::fclose(f);
    return 0;
}

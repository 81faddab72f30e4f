/*
 * ssim_host.cpp -- TEST INFRASTRUCTURE: the arithmetic of the SSIM measurement (pngloss_amd/csrc/pl_ssim_core.h, shared with the HIP kernels
 * pl_ssim and pl_ssim_visible) on the CPU: per tile the kernel's two thread loops run for tid = 0 .. nthreads - 1 over a table the size of the
 * kernel's LDS one, the partial records merged by channel, the record printed.  Built with -fsanitize=address,undefined and run by
 * tests/test_ssim_host.py, which compares every record with a restatement in Python integers.  Never shipped.
 *
 *   ssim_host CASES
 * CASES: uint64 count, then per case uint64 { width, height, a_offset, b_offset, nthreads, blocks, visible } and width * height words of a, then
 * of b.  Each image gets a heap block of its own that starts a_offset / b_offset bytes behind a 16-byte boundary and ends with its last pixel, so
 * a load past an image is a report; the table is a heap block of exactly PLS_TILE_CELLS * 4 entries.
 *   blocks = 0   every tile on a table poisoned with 0xA5 just before it, a fresh partial record per (tile, tid): what a tile does not write,
 *                it must not read
 *   blocks = B   the kernel's workgroups: for each b < B the table is poisoned ONCE, then tiles b, b + B, ... run over it with nothing cleared
 *                between them -- a tile sees the cells of the tiles before it wherever it writes none, as the LDS table of a workgroup does --
 *                and thread tid keeps one partial record across its workgroup's tiles
 *   visible      0: the plain instantiation (pl_ssim); 1: the visible one (pl_ssim_visible), which counts the windows as well
 * Prints per case one line: windows sum_q16[0..3] min_q16[0..3] reserved.
 *
 *   ssim_host grid N MAX_TILES [N MAX_TILES ...]
 * The launch shape of pl_ssim.hip: prints PLS_MAX_IMAGES on one line, then per (N, MAX_TILES) pls_grid_blocks(N, MAX_TILES); N >= 1.
 */
#include "../../pngloss_amd/csrc/pl_ssim_core.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
    std::printf("%zu\n", PLS_MAX_IMAGES);
    for (int k = 2; k < argc; k += 2) {
        const uint64_t n = std::strtoull(argv[k], nullptr, 10), max_tiles = std::strtoull(argv[k + 1], nullptr, 10);
        if (!n) return 2;
        std::printf("%zu\n", pls_grid_blocks((size_t)n, max_tiles));
    }
    return 0;
}

/* one tile: every thread's cells, then (the kernel's barrier) every thread's windows into parts[tid] */
template <bool Visible>
static void run_tile(PlsCell *table, std::vector<PlsPart> &parts, const uint32_t *a, const uint32_t *b, uint32_t width, uint32_t height, const PlsGeom &g,
                     uint64_t tile)
{
    const uint32_t nthreads = (uint32_t)parts.size();
    for (uint32_t tid = 0; tid < nthreads; tid++) pls_thread_cells<Visible>(table, a, b, width, height, g, tile, tid, nthreads);
    for (uint32_t tid = 0; tid < nthreads; tid++) pls_thread_windows<Visible>(parts[tid], table, g, tile, tid, nthreads);
}

/* the partial records of a workgroup (or of one tile) into the record, by channel; false: a pair of another channel than 3 counted a window */
template <bool Visible>
static bool merge(PlSsimRecord &r, std::vector<PlsPart> &parts)
{
    for (uint32_t tid = 0; tid < parts.size(); tid++) {
        const PlsPart &p = parts[tid];
        if ((!Visible || (tid & 3) != 3) && p.windows) return false;
        r.sum_q16[tid & 3] += p.sum;
        if (p.mn < r.min_q16[tid & 3]) r.min_q16[tid & 3] = p.mn;
        r.windows += p.windows;
        parts[tid] = pls_part();
    }
    return true;
}

template <bool Visible>
static bool run_case(PlSsimRecord &r, PlsCell *table, const uint32_t *a, const uint32_t *b, uint32_t width, uint32_t height, uint32_t nthreads, uint64_t blocks)
{
    const size_t table_bytes = sizeof(PlsCell) * PLS_TILE_CELLS * 4;
    const PlsGeom g = pls_geom(width, height);
    std::vector<PlsPart> parts(nthreads, pls_part());
    r = Visible ? pls_record_begin_visible() : pls_record_begin(width, height);
    if (!blocks) {
        for (uint64_t tile = 0; tile < g.tiles; tile++) {
            std::memset(table, 0xA5, table_bytes);
            run_tile<Visible>(table, parts, a, b, width, height, g, tile);
            if (!merge<Visible>(r, parts)) return false;
        }
        return true;
    }
    for (uint64_t wg = 0; wg < blocks; wg++) {
        std::memset(table, 0xA5, table_bytes);
        for (uint64_t tile = wg; tile < g.tiles; tile += blocks) run_tile<Visible>(table, parts, a, b, width, height, g, tile);
        if (!merge<Visible>(r, parts)) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::strcmp(argv[1], "grid") == 0) return grid(argc, argv);
    FILE *f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    uint64_t count = 0;
    if (!f || std::fread(&count, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t head[7];
        if (std::fread(head, 8, 7, f) != 7 || head[2] % 4 || head[3] % 4 || !head[4] || head[4] % 4 || head[6] > 1) return 2;
        const uint32_t width = (uint32_t)head[0], height = (uint32_t)head[1], nthreads = (uint32_t)head[4];
        void *base_a = nullptr, *base_b = nullptr, *base_t = nullptr;
        const uint32_t *a = block(f, head[0] * head[1], head[2], &base_a), *b = block(f, head[0] * head[1], head[3], &base_b);
        if (!a || !b || posix_memalign(&base_t, 16, sizeof(PlsCell) * PLS_TILE_CELLS * 4) != 0) return 2;
        PlsCell *table = static_cast<PlsCell *>(base_t);
        PlSsimRecord r;
        if (!(head[6] ? run_case<true>(r, table, a, b, width, height, nthreads, head[5]) : run_case<false>(r, table, a, b, width, height, nthreads, head[5]))) return 4;
        std::printf("%" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d %d %" PRIu64 "\n", r.windows, r.sum_q16[0], r.sum_q16[1], r.sum_q16[2],
                    r.sum_q16[3], r.min_q16[0], r.min_q16[1], r.min_q16[2], r.min_q16[3], r.reserved);
        std::free(base_a);
        std::free(base_b);
        std::free(base_t);
    }
    std::fclose(f);
    return 0;
}

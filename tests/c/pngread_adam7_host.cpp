/*
 * pngread_adam7_host.cpp -- TEST INFRASTRUCTURE: the device PNG reader's handling of Adam7-interlaced files on the CPU.  Built on the
 * pass geometry (pr_adam7_pass / pr_adam7_bytes) and the pixel arithmetic (pr_recon, pr_expand) of pngloss_amd/csrc/pl_pngread_core.h,
 * which the kernel set-up and the kernel use too: every pass is unfiltered row by row on its own (its first row sees a zero row above it)
 * and each of its pixels is stored at its place in the image.  The CPU suite checks it against the fixtures the real reference reader
 * produced (tests/golden/png_read_adam7_cases.npz); the GPU tests use it as the expectation on random scanlines.  Never shipped.
 */
#include "../../pngloss_amd/csrc/pl_pngread_core.h"

#include <vector>

/* one filtered image (a pass, or a whole non-interlaced file) of w x h pixels -> rgba at (x0 + x * dx, y0 + y * dy) of a pitch-wide image */
static int decode_image(const PrFormat &F, const unsigned char *scan, uint32_t w, uint32_t h, uint32_t rowbytes, uint32_t x0, uint32_t y0,
                        uint32_t dx, uint32_t dy, uint32_t pitch, unsigned char *rgba)
{
    std::vector<uint8_t> prev(rowbytes, 0), cur(rowbytes, 0);
    for (uint32_t y = 0; y < h; y++) {
        const unsigned char *src = scan + (size_t)y * (rowbytes + 1);
        const int ft = src[0];
        if (ft > 4) return 25;
        for (uint32_t i = 0; i < rowbytes; i++) {
            const int a = i >= F.bppf ? cur[i - F.bppf] : 0, b = prev[i], c = i >= F.bppf ? prev[i - F.bppf] : 0;
            cur[i] = (uint8_t)pr_recon(ft, src[1 + i], a, b, c);
        }
        for (uint32_t x = 0; x < w; x++) {
            const uint32_t v = pr_expand(F, cur.data(), x);
            unsigned char *d = rgba + (((size_t)(y0 + y * dy)) * pitch + x0 + (size_t)x * dx) * 4;
            d[0] = (unsigned char)v; d[1] = (unsigned char)(v >> 8); d[2] = (unsigned char)(v >> 16); d[3] = (unsigned char)(v >> 24);
        }
        prev.swap(cur);
    }
    return 0;
}

/* scanlines: nbytes inflated bytes (must be pr_scanline_bytes of the image).  Returns 0, 4 (not a PNG format / wrong size) or 25 (a filter type beyond 4) */
extern "C" int pngread_adam7_decode(const unsigned char *scanlines, uint64_t nbytes, uint32_t width, uint32_t height, int color_type, int depth,
                                    int interlace, const unsigned char *plte, uint32_t plte_entries, const unsigned char *trns, uint32_t trns_bytes,
                                    unsigned char *rgba)
{
    PrFormat F;
    if (interlace < 0 || interlace > 1 || !pr_format(F, width, height, color_type, depth, plte, plte_entries, trns, trns_bytes)) return 4;
    if (nbytes != pr_scanline_bytes(width, height, color_type, depth, interlace)) return 4;
    if (!interlace) return decode_image(F, scanlines, width, height, F.rowbytes, 0, 0, 1, 1, width, rgba);
    uint64_t off[PR_ADAM7_PASSES];
    pr_adam7_bytes(width, height, color_type, depth, off);
    for (int p = 0; p < PR_ADAM7_PASSES; p++) {
        const PrPass s = pr_adam7_pass(p, width, height, color_type, depth);
        if (!s.bytes) continue;
        const int rc = decode_image(F, scanlines + off[p], s.width, s.height, s.rowbytes, s.x0, s.y0, s.dx, s.dy, width, rgba);
        if (rc) return rc;
    }
    return 0;
}

/* the helpers as such, for the geometry test: out = x0, y0, dx, dy, width, height, rowbytes, bytes of pass p */
extern "C" void pngread_adam7_pass(int p, uint32_t width, uint32_t height, int color_type, int depth, uint64_t out[8])
{
    const PrPass s = pr_adam7_pass(p, width, height, color_type, depth);
    out[0] = s.x0; out[1] = s.y0; out[2] = s.dx; out[3] = s.dy; out[4] = s.width; out[5] = s.height; out[6] = s.rowbytes; out[7] = s.bytes;
}

extern "C" uint64_t pngread_adam7_total(uint32_t width, uint32_t height, int color_type, int depth, uint64_t off[7])
{
    return pr_adam7_bytes(width, height, color_type, depth, off);
}

/*
 * seg_sizes_main.cpp -- TEST INFRASTRUCTURE: the segment engine's kernel bodies (tests/c/seg_host.cpp) on the workspace the LIBRARY lays out
 * (pngloss_amd/csrc/pl_plan.h: pl_seg_layout, pl_seg_bind -- every array a heap block of exactly its bytes) against the CPU restatement
 * (oracle/pngloss_port.c), as a program of its own under -fsanitize=address,undefined: an array the library makes too small, or a pointer bound to
 * the wrong array, is a report here before it is a fault on the device.  Built and run by tests/test_seg_host.py; never shipped.
 *
 * The smallest shapes at which a size or a binding can be wrong: one segment (1), SEG_L pixels and one more (32, 33), a second group of SEG_GRP
 * segments and a third commit workgroup (513); a state set within the lanes (19, 2) and two seeded ones, which have no `maps` at all (85, 1), (255, 1).
 */
#include "../../oracle/pngloss_port.h"

#include <cstdio>
#include <cstring>
#include <vector>

extern "C" void pngloss_synth_rgba(unsigned char *rgba, uint32_t width, uint32_t height, int mode, uint64_t frame);
extern "C" int seg_host_optimize(unsigned char *rgba, uint32_t W, uint32_t H, unsigned char *row_filters, unsigned strength, long bleed, uint32_t *stats);

int main()
{
    static const uint32_t widths[] = { 1, 32, 33, 513 };
    static const struct { unsigned s; long b; } settings[] = { { 19, 2 }, { 85, 1 }, { 255, 1 } };
    int bad = 0, k = 0;
    for (uint32_t w : widths)
        for (const auto &st : settings) {
            const uint32_t h = 3 + (uint32_t)(k & 1);
            const int mode = k++ % 6;
            std::vector<unsigned char> img((size_t)w * h * 4), got, gf(h, 0), wf(h, 0);
            pngloss_synth_rgba(img.data(), w, h, mode, 0);
            got = img;
            uint32_t stats[8] = {};
            const int rc = seg_host_optimize(got.data(), w, h, gf.data(), st.s, st.b, stats);
            std::vector<unsigned char *> rows(h);
            for (uint32_t y = 0; y < h; y++) rows[y] = img.data() + (size_t)y * w * 4;
            const int prc = port_optimize_with_rows(rows.data(), w, h, wf.data(), false, (uint_fast8_t)st.s, (int_fast16_t)st.b);
            const bool same = rc == 0 && prc == 0 && got == img && gf == wf;
            std::printf("%u x %u mode %d strength %u bleed %ld: %s (%u attempts)\n", w, h, mode, st.s, st.b, same ? "equal" : "DIFFERENT", stats[0]);
            if (!same) bad++;
        }
    return bad ? 1 : 0;
}

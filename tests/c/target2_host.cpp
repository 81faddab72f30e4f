/*
 * target2_host.cpp -- TEST INFRASTRUCTURE: what pngloss_amd/csrc/pl_target.h adds for pngloss_hip_optimize_batch_target2 -- the check of a
 * pngloss_hip_target2, the acceptance rule with the SSIM condition and the arena layout with the SSIM tables -- on the CPU.  Built with
 * -fsanitize=address,undefined and run by tests/test_ssim_host.py against the rule restated in Python (tests/util_ssim.py).  Never shipped.
 *
 *   target2_host COMMANDS        one answer line per command line:
 *     C psnr max_abs max_strength ssim                 pl_target_check2's return code (doubles as 16 hex digits of their bits)
 *     A psnr max_abs ssim status bpp pixels sq[4] mx[4] windows sum[4]      pl_target_accept2: 1 or 0
 *     L host ssim_job_bytes ssim_record_bytes w h [w h ...]                 pl_target_layout: total moves jobs records ssim_jobs ssim_records, then per
 *                                                                           image orig best best_filters img filters
 */
#include "../../pngloss_amd/csrc/pl_target.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

static double bits(const std::string &hex)
{
    const uint64_t u = std::strtoull(hex.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char buf[4096];
    while (std::fgets(buf, sizeof buf, f)) {
        std::istringstream in(buf);
        std::string cmd, p, s;
        in >> cmd;
        if (cmd == "C") {
            pngloss_hip_target2 t{};
            in >> p >> t.max_abs_error >> t.max_strength >> s;
            t.min_psnr_db = bits(p); t.min_ssim = bits(s);
            std::printf("%d\n", pl_target_check2(&t));
        } else if (cmd == "A") {
            pngloss_hip_target2 t{};
            pngloss_hip_distortion rec{};
            pngloss_hip_ssim sr{};
            int32_t status = 0;
            uint32_t bpp = 0;
            in >> p >> t.max_abs_error >> s >> status >> bpp >> rec.pixels;
            t.min_psnr_db = bits(p); t.min_ssim = bits(s); t.max_strength = 19;
            for (int c = 0; c < 4; c++) in >> rec.sq_err[c];
            for (int c = 0; c < 4; c++) in >> rec.max_abs[c];
            in >> sr.windows;
            for (int c = 0; c < 4; c++) in >> sr.sum_q16[c];
            rec.changed_pixels = 1;
            std::printf("%d\n", pl_target_accept2(t, rec, sr, status, bpp) ? 1 : 0);
        } else if (cmd == "L") {
            int host = 0;
            size_t sj = 0, sr = 0;
            in >> host >> sj >> sr;
            std::vector<uint32_t> w, h;
            for (uint32_t a, b; in >> a >> b;) { w.push_back(a); h.push_back(b); }
            const PlTargetLayout lay = sj || sr ? pl_target_layout(w, h, host != 0, 24, 32, 64, sj, sr) : pl_target_layout(w, h, host != 0, 24, 32, 64);
            std::printf("%zu %zu %zu %zu %zu %zu", lay.total, lay.moves, lay.jobs, lay.records, lay.ssim_jobs, lay.ssim_records);
            for (const PlTargetImage &m : lay.image) std::printf(" %zu %zu %zu %zu %zu", m.orig, m.best, m.best_filters, m.img, m.filters);
            std::printf("\n");
        } else return 2;
    }
    std::fclose(f);
    return 0;
}

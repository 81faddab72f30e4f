/* tests/c/cli_report_host.c -- test driver for pngloss_amd/cli/cli_report.c, linked with libpngloss_hip.so for pngloss_hip_psnr_db and
 * pngloss_hip_ssim_mean (host arithmetic: no device).  Reads one hand-made record per line from stdin and prints the tool's line about it:
 *   distortion BPP VISIBLE pixels changed sq_err[4] max_abs[4]
 *   ssim HAVE SEARCH BPP VISIBLE windows sum_q16[4] min_q16[4]          HAVE 0: the file has no record; SEARCH 0 none, 1 quality, 2 size
 *   strength STRENGTH PROBES
 *   indexed colors indexed_bytes entries trns_entries truecolor_bytes
 *   budget NAME budget written strength
 *   mask BPP                                                            prints the channel mask in hex */
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "cli_report.h"

int main(void)
{
    char in[1024], line[1024], name[512];
    while (fgets(in, sizeof in, stdin)) {
        unsigned bpp, visible, have, search, a, b;
        size_t x, y;
        pngloss_hip_distortion d;
        pngloss_hip_ssim r;
        pngloss_hip_palette p;
        memset(&r, 0, sizeof r);
        memset(&p, 0, sizeof p);
        line[0] = 0;
        if (sscanf(in, "distortion %u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &bpp, &visible,
                   &d.pixels, &d.changed_pixels, &d.sq_err[0], &d.sq_err[1], &d.sq_err[2], &d.sq_err[3], &d.max_abs[0], &d.max_abs[1], &d.max_abs[2], &d.max_abs[3]) == 12)
            cli_report_distortion(line, sizeof line, &d, bpp, visible);
        else if (sscanf(in, "ssim %u %u %u %u %" SCNu64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &have, &search, &bpp,
                        &visible, &r.windows, &r.sum_q16[0], &r.sum_q16[1], &r.sum_q16[2], &r.sum_q16[3], &r.min_q16[0], &r.min_q16[1], &r.min_q16[2], &r.min_q16[3]) == 13)
            cli_report_ssim(line, sizeof line, have ? &r : NULL, (enum cli_search)search, bpp, visible);
        else if (sscanf(in, "strength %u %u", &a, &b) == 2) cli_report_strength(line, sizeof line, a, b);
        else if (sscanf(in, "indexed %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64, &p.colors, &p.indexed_bytes, &p.entries, &p.trns_entries, &p.truecolor_bytes) == 5)
            cli_report_indexed(line, sizeof line, &p);
        else if (sscanf(in, "budget %511s %zu %zu %u", name, &x, &y, &a) == 4) cli_report_budget_missed(line, sizeof line, name, x, y, a);
        else if (sscanf(in, "mask %u", &bpp) == 1) snprintf(line, sizeof line, "%x\n", cli_stored_channel_mask(bpp));
        else return 2;
        printf("%s--\n", line);            /* a separator of its own line: an empty answer and a missing newline both show */
    }
    return 0;
}

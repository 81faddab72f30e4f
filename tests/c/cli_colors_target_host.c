/* tests/c/cli_colors_target_host.c -- test driver for the switches --colors-psnr and --colors-max-error of pngloss_amd/cli/cli_options.c (no libpng;
 * the report lines ask the device library for its PSNR formula only), as tests/c/cli_colors_host.c is for --colors.  A refused vector leaves its
 * message on stderr and its code as the exit status; one that passes prints the fields the switches set or leave alone, one "name=value" per line,
 * and exits 0.
 * With "report colors reached probes max_colors pixels sq_err changed" it prints the -v line of cli_report.c for the colour count a search chose
 * (sq_err: the squared error, all of it in channel 0), and with "missed name max_colors" the warning for a target that was not reached.
 * With "usage" it prints the usage text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cli_options.h"
#include "cli_report.h"

int main(int argc, char **argv)
{
    char line[512];
    if (argc == 9 && !strcmp(argv[1], "report")) {
        pngloss_hip_quant_target_report r;
        memset(&r, 0, sizeof r);
        r.colors = (uint32_t)atoi(argv[2]); r.reached = (uint32_t)atoi(argv[3]); r.probes = (uint32_t)atoi(argv[4]);
        r.probe_distortion.pixels = strtoull(argv[6], NULL, 10);
        r.probe_distortion.sq_err[0] = strtoull(argv[7], NULL, 10);
        r.probe_distortion.changed_pixels = strtoull(argv[8], NULL, 10);
        cli_report_chosen_colors(line, sizeof line, &r, (unsigned)atoi(argv[5]));
        fputs(line, stdout);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "missed")) {
        cli_report_colors_missed(line, sizeof line, argv[2], (unsigned)atoi(argv[3]));
        fputs(line, stdout);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "usage")) { fputs(cli_usage_text, stdout); return 0; }
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (!o.version && !o.missing && !o.help) rc = cli_options_check(&o, stderr);
    if (rc != SUCCESS) return rc;
    printf("have_colors=%d\ncolors=%lu\nhave_colors_psnr=%d\ncolors_psnr=%g\nhave_colors_max_error=%d\ncolors_max_error=%lu\ndither=%d\nstrength=%lu\nindexed=%d\n"
           "gpu_deflate=%d\ndistortion=%d\nverbose=%d\n", o.have_colors, o.colors, o.have_colors_psnr, o.have_colors_psnr ? o.colors_psnr : 0.0, o.have_colors_max_error,
           o.have_colors_max_error ? o.colors_max_error : 0ul, o.dither, o.strength, o.indexed, o.gpu_deflate, o.distortion, o.verbose);
    return 0;
}

/* tests/c/cli_colors_visible_host.c -- test driver for the switch --colors-visible of pngloss_amd/cli/cli_options.c (no libpng, no device library), as
 * tests/c/cli_dither_host.c is for --dither.  A refused vector leaves its message on stderr and its code as the exit status; one that passes prints
 * the fields the switch sets or leaves alone, one "name=value" per line, and exits 0.
 * With "report colors_in entries exact" it prints the -v lines of cli_report.c for a file of a --colors --colors-visible run: the colours, then the
 * line of the space.  With "distortion pixels changed sq max visible" it prints the --distortion line.  With "usage" it prints the usage text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cli_options.h"
#include "cli_report.h"

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "report")) {
        pngloss_hip_quant_report q;
        char line[256];
        memset(&q, 0, sizeof q);
        q.colors_in = (uint32_t)atoi(argv[2]); q.entries = (uint32_t)atoi(argv[3]); q.exact = (uint32_t)atoi(argv[4]);
        cli_report_quant(line, sizeof line, &q);
        fputs(line, stdout);
        cli_report_colors_space(line, sizeof line, &q);
        fputs(line, stdout);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "distortion")) {
        pngloss_hip_distortion d;
        char line[256];
        memset(&d, 0, sizeof d);
        d.pixels = strtoull(argv[2], NULL, 10); d.changed_pixels = strtoull(argv[3], NULL, 10);
        for (int c = 0; c < 4; c++) { d.sq_err[c] = strtoull(argv[4], NULL, 10); d.max_abs[c] = (uint32_t)atoi(argv[5]); }
        cli_report_distortion(line, sizeof line, &d, 4, atoi(argv[6]) != 0);
        fputs(line, stdout);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "usage")) { fputs(cli_usage_text, stdout); return 0; }
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (!o.version && !o.missing && !o.help) rc = cli_options_check(&o, stderr);
    if (rc != SUCCESS) return rc;
    printf("colors_visible=%d\nvisible=%d\ndither=%d\nhave_colors=%d\ncolors=%lu\nhave_colors_psnr=%d\nhave_colors_max_error=%d\nstrength=%lu\nindexed=%d\ngpu_deflate=%d\n"
           "distortion=%d\nverbose=%d\n", o.colors_visible, o.visible, o.dither, o.have_colors, o.colors, o.have_colors_psnr, o.have_colors_max_error, o.strength,
           o.indexed, o.gpu_deflate, o.distortion, o.verbose);
    return 0;
}

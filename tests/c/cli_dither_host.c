/* tests/c/cli_dither_host.c -- test driver for the switch --dither of pngloss_amd/cli/cli_options.c (no libpng, no device library), as
 * tests/c/cli_colors_host.c is for --colors.  A refused vector leaves its message on stderr and its code as the exit status; one that passes prints
 * the fields the switch sets or leaves alone, one "name=value" per line, and exits 0.
 * With "report colors_in entries exact" it prints the -v lines of cli_report.c for a file of a --colors --dither run: the colours, then the dither line.
 * With "usage" it prints the usage text. */
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
        cli_report_dither(line, sizeof line, &q);
        fputs(line, stdout);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "usage")) { fputs(cli_usage_text, stdout); return 0; }
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (!o.version && !o.missing && !o.help) rc = cli_options_check(&o, stderr);
    if (rc != SUCCESS) return rc;
    printf("dither=%d\nhave_colors=%d\ncolors=%lu\nhave_strength=%d\nstrength=%lu\nindexed=%d\ngpu_deflate=%d\ndistortion=%d\nverbose=%d\n", o.dither, o.have_colors,
           o.colors, o.have_strength, o.strength, o.indexed, o.gpu_deflate, o.distortion, o.verbose);
    return 0;
}

/* tests/c/cli_index_depth_host.c -- test driver for the switch --index-depth of pngloss_amd/cli/cli_options.c (no libpng, no device library), as
 * tests/c/cli_colors_visible_host.c is for --colors-visible.  A refused vector leaves its message on stderr and its code as the exit status; one
 * that passes prints the fields the switch sets or leaves alone, one "name=value" per line, and exits 0.
 * With "report bit_depth min_depth indexed8_bytes packed_bytes" it prints the -v line of cli_report.c for a file kept at that depth (nothing for a
 * file at 8 bits or truecolour).  With "usage" it prints the usage text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cli_options.h"
#include "cli_report.h"

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "report")) {
        pngloss_hip_index_depth r;
        char line[256];
        memset(&r, 0, sizeof r);
        r.bit_depth = (uint32_t)atoi(argv[2]); r.min_depth = (uint32_t)atoi(argv[3]);
        r.indexed8_bytes = strtoull(argv[4], NULL, 10); r.packed_bytes = strtoull(argv[5], NULL, 10);
        cli_report_index_depth(line, sizeof line, &r);
        fputs(line, stdout);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "usage")) { fputs(cli_usage_text, stdout); return 0; }
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (!o.version && !o.missing && !o.help) rc = cli_options_check(&o, stderr);
    if (rc != SUCCESS) return rc;
    printf("have_index_depth=%d\nindex_depth=%s\nindexed=%d\nhave_colors=%d\ncolors=%lu\ndither=%d\nstrength=%lu\ngpu_deflate=%d\nverbose=%d\n", o.have_index_depth,
           o.index_depth ? o.index_depth : "", o.indexed, o.have_colors, o.colors, o.dither, o.strength, o.gpu_deflate, o.verbose);
    return 0;
}

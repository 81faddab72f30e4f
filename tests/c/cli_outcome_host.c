/* tests/c/cli_outcome_host.c -- test driver for pngloss_amd/cli/cli_outcome.h (header only: nothing is linked): every function over its whole
 * domain, one line per point, inputs first and the answer behind "->".  tests/test_cli_options_host.py holds the expected tables.
 * usage: cli_outcome_host                              the grids
 *        cli_outcome_host budget PERCENT VALUE SIZE    cli_file_budget;   cli_outcome_host stream LARGEST    cli_stream_budget */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cli_outcome.h"

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "budget")) return printf("%zu\n", cli_file_budget(atoi(argv[2]) != 0, strtoull(argv[3], NULL, 10), (size_t)strtoull(argv[4], NULL, 10))) < 0;
    if (argc == 3 && !strcmp(argv[1], "stream")) return printf("%llu\n", (unsigned long long)cli_stream_budget((size_t)strtoull(argv[2], NULL, 10))) < 0;
    static const int codes[] = { PNGLOSS_SUCCESS, PNGLOSS_INTERNAL_ABORT, PNGLOSS_HIP_ERROR, PNGLOSS_OUT_OF_MEMORY_ERROR };
    static const enum cli_search searches[] = { CLI_SEARCH_NONE, CLI_SEARCH_QUALITY, CLI_SEARCH_SIZE };
    static const int statuses[] = { 0, PNGLOSS_INTERNAL_ABORT };       /* results[k].status of one image */
    for (int c = 0; c < 4; c++)
        for (int s = 0; s < 2; s++) printf("optimise %d %d -> %d\n", codes[c], statuses[s], cli_status_after_optimise(codes[c], statuses[s]));
    for (int m = 0; m < 3; m++)
        for (int asked = 0; asked < 2; asked++)
            for (int tssim = 0; tssim < 2; tssim++)
                for (int c = 0; c < 4; c++)
                    for (int last = 0; last < 2; last++)
                        printf("records %d %d %d %d %d -> %d %d %d\n", (int)searches[m], asked, tssim, codes[c], last, cli_have_distortion(searches[m], asked, codes[c], last),
                               cli_have_ssim(searches[m], asked, tssim, codes[c], last), cli_have_palette(searches[m], asked, last));
    for (int type = 0; type < 2; type++)
        for (int have = 0; have < 2; have++)
            for (int c = 0; c < 4; c++) printf("indexed %d %d %d -> %d\n", type ? 3 : 6, have, codes[c], cli_indexed_without_palette(type ? 3 : 6, have, codes[c]));
    for (int setup = 0; setup < 2; setup++)
        for (int batch = 0; batch < 2; batch++)
            for (int s = 0; s < 2; s++)
                for (int explained = 0; explained < 2; explained++) {
                    const int setup_rc = setup ? PNGLOSS_OUT_OF_MEMORY_ERROR : PNGLOSS_SUCCESS, batch_rc = batch ? PNGLOSS_HIP_ERROR : PNGLOSS_SUCCESS;
                    const int st = s ? PNGLOSS_INVALID_ARGUMENT : 0;      /* a code of its own, so that the table tells whose code came out */
                    printf("read %d %d %d %d -> %d\n", setup_rc, batch_rc, st, explained, cli_status_after_device_read(setup_rc, batch_rc, st, explained));
                }
    return 0;
}

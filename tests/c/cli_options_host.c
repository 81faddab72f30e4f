/* tests/c/cli_options_host.c -- test driver for pngloss_amd/cli/cli_options.c on its own (no libpng, no device library): parse and check argv the
 * way the tool's main does.  A refused vector leaves its message on stderr and its code as the exit status; a vector that passes prints every
 * field of the record, one "name=value" per line, and exits 0.  --version, --help and a missing command line, which the tool answers before the
 * check, print the record too. */
#include <stdio.h>
#include "cli_options.h"

int main(int argc, char **argv)
{
    struct cli_options o;
    pngloss_error rc = cli_options_parse(argc, argv, &o, stderr);
    if (rc != SUCCESS) return rc;
    if (!o.version && !o.missing && !o.help) rc = cli_options_check(&o, stderr);
    if (rc != SUCCESS) return rc;
    static const char *const search[] = { "none", "quality", "size", "both" };
    printf("extension=%s\noutput_path=%s\nfiles=", o.extension ? o.extension : "", o.output_path ? o.output_path : "");
    for (unsigned i = 0; i < o.num_files; i++) printf(i ? " %s" : "%s", o.files[i]);
    printf("\nstrength=%lu\nbleed=%lu\nnum_files=%u\n", o.strength, o.bleed, o.num_files);
    printf("from_stdin=%d\nto_stdout=%d\nforce=%d\nskip_if_larger=%d\nstrip=%d\nhelp=%d\nversion=%d\nmissing=%d\nverbose=%d\n", o.from_stdin, o.to_stdout, o.force,
           o.skip_if_larger, o.strip, o.help, o.version, o.missing, o.verbose);
    printf("gpu_deflate=%d\ngpu_read=%d\ndistortion=%d\nssim=%d\nvisible=%d\nindexed=%d\nsearch=%s\n", o.gpu_deflate, o.gpu_read, o.distortion, o.ssim, o.visible,
           o.indexed, search[o.search]);
    printf("target_psnr=%.17g\nhave_max_error=%d\nmax_error=%lu\nhave_target_ssim=%d\ntarget_ssim=%.17g\nsize_percent=%d\nsize_value=%llu\n", o.target_psnr,
           o.have_max_error, o.max_error, o.have_target_ssim, o.target_ssim, o.size_percent, o.size_value);
    return 0;
}

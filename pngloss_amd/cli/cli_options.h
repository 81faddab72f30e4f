/* cli_options.h -- the command line of the pngloss tool, parsed and checked.  Plain C over getopt_long: no libpng, no device library; the status
 * codes come from png_bridge.h.  tests/c/cli_options_host.c runs it on its own. */
#ifndef PNGLOSS_AMD_CLI_OPTIONS_H
#define PNGLOSS_AMD_CLI_OPTIONS_H

#include <stdbool.h>
#include <stddef.h>
#include <stdio.h>

#include "png_bridge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How each file's strength is found.  Derived once, when the arguments have been read. */
enum cli_search {
    CLI_SEARCH_NONE,      /* -s is the strength of every file */
    CLI_SEARCH_QUALITY,   /* --target-psnr / --max-error / --target-ssim: searched per file, -s is the upper bound */
    CLI_SEARCH_SIZE,      /* --target-size: searched per file from a byte budget for the written file, -s is the upper bound */
    CLI_SEARCH_BOTH,      /* both kinds were asked for: cli_options_check refuses it, so nothing behind the check sees this value */
};

struct cli_options {
    const char *extension;     /* --ext; NULL: CLI_DEFAULT_EXTENSION */
    const char *output_path;
    char *const *files;
    unsigned long strength, bleed;
    unsigned num_files;
    bool from_stdin, to_stdout, force, skip_if_larger, strip, help, version, missing, verbose;
    bool gpu_deflate;          /* --gpu-deflate: IDAT data compressed on the device instead of by zlib level 9 (--indexed and --target-size imply it) */
    bool gpu_read;             /* --gpu-read: inverse filters + expansion to RGBA8 on the device (inflate stays zlib on the decode threads) */
    bool distortion;           /* --distortion: one line per written file saying how far its pixels are from the input's (measured on the device) */
    bool ssim;                 /* --ssim: one more line per written file: mean and worst-window SSIM against the input's pixels (measured on the device) */
    bool visible;              /* --visible: --distortion, --ssim and the --target searches measure over visible pixels (the library's option "measure") */
    bool indexed;              /* --indexed: a result of at most 256 colours is written as a palette file where that file is smaller (the library's option "indexed") */
    bool have_colors;          /* --colors N: every image is quantised to at most N colours first (pngloss_hip_multi_quantize_batch_host), then written at */
    unsigned long colors;      /* strength 0 with --indexed: the palette is the lossy step.  Not in the usage text (DESIGN.md 9.1b says why) */
    bool dither;               /* --dither: --colors remaps with Floyd-Steinberg error diffusion (pngloss_hip_multi_quantize_batch_host2).  Not in the usage text either */
    /* --colors-psnr DB, --colors-max-error E: with --colors M, the colour count is searched per file, at most M: the fewest colours -- by the rule of
     * include/pngloss_hip_quant_target.h -- that keep DB decibels of PSNR over all four channels, a largest channel error of E, or both
     * (pngloss_hip_multi_quantize_batch_host_target).  Not in the usage text either.  A value that does not parse is remembered (*_ok) and refused by
     * cli_options_check behind every older rule */
    bool have_colors_psnr, colors_psnr_ok;
    double colors_psnr;
    bool have_colors_max_error, colors_max_error_ok;
    unsigned long colors_max_error;
    /* --colors-visible: --colors searches its palette on alpha-premultiplied pixels (the *3 calls of include/pngloss_hip_quant_space.h at space 1), and
     * the record behind --distortion and the colour-count search is the visible-mode one.  Not in the usage text either */
    bool colors_visible;
    /* --index-depth auto|min|8: with --indexed or --colors, the bit depth of a palette file of at most 16 colours (the library's option
     * "index_depth": 8 bits as without the switch, the smallest file of 8 bits and the packed depth, or the packed depth alone).  Not in the usage
     * text either.  A value that is none of the three is remembered (index_depth_ok) and refused by cli_options_check behind every older rule */
    bool have_index_depth, index_depth_ok;
    const char *index_depth;
    bool have_strength;        /* -s was given */
    enum cli_search search;
    double target_psnr;        /* 0: no PSNR condition */
    bool have_max_error;
    unsigned long max_error;   /* 0: no condition */
    bool have_target_ssim;     /* --target-ssim: a condition of the quality search, like --target-psnr */
    double target_ssim;        /* 0: no SSIM condition */
    bool size_percent;         /* --target-size given as a percentage of each input file's size */
    unsigned long long size_value;   /* bytes, or percent */
};

#define CLI_DEFAULT_EXTENSION "-loss.png"

extern const char cli_usage_text[];

/* argv into *o (defaults: strength 19, bleed 2).  A malformed argument writes its message to err -- getopt_long writes its own to stderr -- and
 * returns INVALID_ARGUMENT.  Ends by deriving `search`, the implied gpu_deflate and what --colors implies (--indexed, and strength 0 without -s). */
pngloss_error cli_options_parse(int argc, char **argv, struct cli_options *o, FILE *err);

/* Every rule between the arguments, in the order in which a user meets their messages: the first one broken writes its message to err and gives
 * the exit code.  After "No input files specified." (MISSING_ARGUMENT) the caller prints the usage text. */
pngloss_error cli_options_check(const struct cli_options *o, FILE *err);

#ifdef __cplusplus
}
#endif
#endif

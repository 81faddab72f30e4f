/* cli_options.c -- the option table, the usage text and the rules between the arguments of the pngloss tool (cli_options.h). */
#include "cli_options.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>

const char cli_usage_text[] =
    "usage:  pngloss [options] -- pngfile [pngfile ...]\n"
    "        pngloss [options] - >stdout <stdin\n\n"
    "options:\n"
    "  -s, --strength 19 how much quality to sacrifice, from 0 to 100 (default 19)\n"
    "  -b, --bleed 2     bleed divider, from 1 (full dithering) to 32767 (none)\n"
    "  -f, --force       overwrite existing output files\n"
    "  -o, --output file destination file path to use instead of --ext\n"
    "  -v, --verbose     print status messages\n"
    "  -q, --quiet       don't print status messages (default, overrides -v)\n"
    "  -V, --version     print version number\n"
    "  --skip-if-larger  only save converted files if they're smaller than original\n"
    "  --ext new.png     set custom suffix/extension for output filenames\n"
    "  --strip           remove optional metadata (default on Mac)\n"
    "  --gpu-deflate     compress the image data on the GPU too (not zlib's bytes, same pixels,\n"
    "                    files several percent smaller than with zlib level 9, much faster)\n"
    "  --gpu-read        undo the PNG scanline filters and expand to RGBA on the GPU (plain or\n"
    "                    Adam7-interlaced files; the others are read with libpng as usual)\n"
    "  --indexed         write a result of at most 256 colours as a palette file (colour type 3) where that\n"
    "                    makes the file smaller: both encodings are compressed on the GPU and the smaller\n"
    "                    file is kept; implies --gpu-deflate; -v prints the colours and both sizes; not\n"
    "                    with --target-size, --target-psnr, --target-ssim or --max-error\n"
    "  --distortion      report how lossy each written file is: PSNR over the stored channels,\n"
    "                    changed pixels, largest channel error (measured on the GPU)\n"
    "  --target-psnr DB  pick each file's strength itself: the search (at most -s, by halving) for a\n"
    "                    result with at least DB decibels of PSNR over the stored channels\n"
    "  --max-error N     the same with a bound on the largest channel error, 1 to 255; both may\n"
    "                    be given (searched on the GPU; -v prints the strength chosen)\n"
    "  --ssim            report each written file's structural similarity to its input: mean and worst\n"
    "                    8x8 window over the stored channels, 1 = identical (measured on the GPU; in a\n"
    "                    strength search only together with --target-ssim)\n"
    "  --target-ssim X   the strength search with a smallest mean SSIM, above 0 and at most 1; combines\n"
    "                    with --target-psnr and --max-error: every condition given must hold\n"
    "  --target-size N   pick each file's strength itself: the smallest (at most -s, by halving) whose\n"
    "                    written file has at most N bytes (suffix k or M: powers of 1024), or P% of\n"
    "                    the input file's size; implies --gpu-deflate; a budget that -s does not\n"
    "                    reach writes the file at -s with a warning; not with the other --target\n"
    "                    switches or --max-error (--ssim has no record in this search)\n"
    "  --visible         measure over visible pixels: --distortion, --ssim, --target-psnr, --max-error and\n"
    "                    --target-ssim then take alpha-premultiplied colour plus alpha, and leave out\n"
    "                    pixels that are fully transparent in the input and in the result; needs one of\n"
    "                    those five; not with --target-size; the written files do not depend on it\n"
    "\n"
    "Lossily compresses PNGs by using more compressible colors that are close enough to the\n"
    "original values; the filter+quantise pass runs on the GPU (all files of a call as one batch).\n"
    "Output names end in \"-loss.png\" or your --ext; with \"-\" the image goes stdin -> stdout.\n"
    "Existing outputs are skipped unless --force is given.\n";

enum { OPT_EXT = 256, OPT_NO_FORCE, OPT_SKIP_LARGER, OPT_STRIP, OPT_GPU_DEFLATE, OPT_GPU_READ, OPT_DISTORTION, OPT_TARGET_PSNR, OPT_MAX_ERROR, OPT_SSIM, OPT_TARGET_SSIM, OPT_TARGET_SIZE, OPT_VISIBLE, OPT_INDEXED, OPT_COLORS, OPT_DITHER, OPT_COLORS_PSNR, OPT_COLORS_MAX_ERROR, OPT_COLORS_VISIBLE, OPT_INDEX_DEPTH };

static bool parse_number(const char *text, unsigned long *out)
{
    char *end;
    unsigned long v = strtoul(text, &end, 10);
    if (end == text || *end) return false;
    *out = v;
    return true;
}

static bool parse_decibels(const char *text, double *out)
{
    char *end;
    double v = strtod(text, &end);
    if (end == text || *end) return false;
    *out = v;
    return true;
}

/* --target-size: N, Nk, NM (powers of 1024) or P% */
static bool parse_size(const char *text, unsigned long long *value, bool *percent)
{
    if (*text < '0' || *text > '9') return false;
    char *end;
    errno = 0;
    unsigned long long v = strtoull(text, &end, 10);
    if (errno == ERANGE) return false;
    *percent = false;
    if (*end == '%') { *percent = true; end++; }
    else if (*end == 'k' || *end == 'K') { if (v > (~0ull >> 10)) return false; v <<= 10; end++; }
    else if (*end == 'M') { if (v > (~0ull >> 20)) return false; v <<= 20; end++; }
    if (*end) return false;
    *value = v;
    return true;
}

static pngloss_error refuse(FILE *err, const char *message)
{
    fputs(message, err);
    return INVALID_ARGUMENT;
}

pngloss_error cli_options_parse(int argc, char **argv, struct cli_options *o, FILE *err)
{
    static const struct option table[] = {
        { "strength", required_argument, NULL, 's' }, { "bleed", required_argument, NULL, 'b' },
        { "force", no_argument, NULL, 'f' },          { "no-force", no_argument, NULL, OPT_NO_FORCE },
        { "output", required_argument, NULL, 'o' },   { "ext", required_argument, NULL, OPT_EXT },
        { "verbose", no_argument, NULL, 'v' },        { "quiet", no_argument, NULL, 'q' },
        { "skip-if-larger", no_argument, NULL, OPT_SKIP_LARGER }, { "strip", no_argument, NULL, OPT_STRIP },
        { "version", no_argument, NULL, 'V' },        { "help", no_argument, NULL, 'h' },
        { "gpu-deflate", no_argument, NULL, OPT_GPU_DEFLATE },
        { "gpu-read", no_argument, NULL, OPT_GPU_READ },
        { "distortion", no_argument, NULL, OPT_DISTORTION },
        { "target-psnr", required_argument, NULL, OPT_TARGET_PSNR },
        { "max-error", required_argument, NULL, OPT_MAX_ERROR },
        { "ssim", no_argument, NULL, OPT_SSIM },
        { "target-ssim", required_argument, NULL, OPT_TARGET_SSIM },
        { "target-size", required_argument, NULL, OPT_TARGET_SIZE },
        { "visible", no_argument, NULL, OPT_VISIBLE },
        { "indexed", no_argument, NULL, OPT_INDEXED },
        { "colors", required_argument, NULL, OPT_COLORS },
        { "dither", no_argument, NULL, OPT_DITHER },
        { "colors-psnr", required_argument, NULL, OPT_COLORS_PSNR },
        { "colors-max-error", required_argument, NULL, OPT_COLORS_MAX_ERROR },
        { "colors-visible", no_argument, NULL, OPT_COLORS_VISIBLE },
        { "index-depth", required_argument, NULL, OPT_INDEX_DEPTH },
        { NULL, 0, NULL, 0 },
    };
    memset(o, 0, sizeof *o);
    o->strength = 19;
    o->bleed = 2;
    bool quality = false, size = false;
    for (int c; (c = getopt_long(argc, argv, "vqfo:Vhs:b:", table, NULL)) != -1;) {
        switch (c) {
        case 'v': o->verbose = true; break;
        case 'q': o->verbose = false; break;
        case 'f': o->force = true; break;
        case OPT_NO_FORCE: o->force = false; break;
        case OPT_EXT: o->extension = optarg; break;
        case OPT_SKIP_LARGER: o->skip_if_larger = true; break;
        case OPT_STRIP: o->strip = true; break;
        case OPT_GPU_DEFLATE: o->gpu_deflate = true; break;
        case OPT_GPU_READ: o->gpu_read = true; break;
        case OPT_DISTORTION: o->distortion = true; break;
        case OPT_TARGET_PSNR:
            if (!parse_decibels(optarg, &o->target_psnr)) return refuse(err, "--target-psnr requires a numeric argument\n");
            quality = true;
            break;
        case OPT_MAX_ERROR:
            if (!parse_number(optarg, &o->max_error)) return refuse(err, "--max-error requires a numeric argument\n");
            quality = o->have_max_error = true;
            break;
        case OPT_SSIM: o->ssim = true; break;
        case OPT_TARGET_SSIM:
            if (!parse_decibels(optarg, &o->target_ssim)) return refuse(err, "--target-ssim requires a numeric argument\n");
            quality = o->have_target_ssim = true;
            break;
        case OPT_TARGET_SIZE:
            if (!parse_size(optarg, &o->size_value, &o->size_percent)) return refuse(err, "--target-size requires a number of bytes (suffix k or M) or a percentage\n");
            size = true;
            break;
        case OPT_VISIBLE: o->visible = true; break;
        case OPT_INDEXED: o->indexed = true; break;
        case OPT_COLORS:
            if (!parse_number(optarg, &o->colors)) return refuse(err, "--colors requires a numeric argument\n");
            o->have_colors = true;
            break;
        case OPT_DITHER: o->dither = true; break;
        case OPT_COLORS_PSNR:
            o->have_colors_psnr = true;
            o->colors_psnr_ok = parse_decibels(optarg, &o->colors_psnr);
            break;
        case OPT_COLORS_MAX_ERROR:
            o->have_colors_max_error = true;
            o->colors_max_error_ok = parse_number(optarg, &o->colors_max_error);
            break;
        case OPT_COLORS_VISIBLE: o->colors_visible = true; break;
        case OPT_INDEX_DEPTH:
            o->have_index_depth = true;
            o->index_depth = optarg;
            o->index_depth_ok = strcmp(optarg, "auto") == 0 || strcmp(optarg, "min") == 0 || strcmp(optarg, "8") == 0;
            break;
        case 'h': o->help = true; break;
        case 'V': o->version = true; break;
        case 'o':
            if (o->output_path) return refuse(err, "--output option can be used only once\n");
            if (strcmp(optarg, "-") == 0) o->to_stdout = true;
            else o->output_path = optarg;
            break;
        case 's':
            if (!parse_number(optarg, &o->strength)) return refuse(err, "-s, --strength requires a numeric argument\n");
            o->have_strength = true;
            break;
        case 'b':
            if (!parse_number(optarg, &o->bleed)) return refuse(err, "-b, --bleed requires a numeric argument\n");
            break;
        default: return INVALID_ARGUMENT;
        }
    }
    if (optind < argc) {
        int first = optind;
        if (first == argc - 1 && strcmp(argv[first], "-") == 0) {   /* lone "-": stdin -> stdout (or -> --output) */
            o->from_stdin = true;
            o->to_stdout = !o->output_path;
        }
        o->num_files = (unsigned)(argc - first);
        o->files = argv + first;
    } else if (optind <= 1) {
        o->missing = true;
    }
    o->search = quality && size ? CLI_SEARCH_BOTH : quality ? CLI_SEARCH_QUALITY : size ? CLI_SEARCH_SIZE : CLI_SEARCH_NONE;
    /* --indexed chooses between two streams of the device deflate; --target-size budgets the file the device deflate writes: zlib-9's size is not
     * what the device measures */
    /* --colors makes the palette that --indexed writes, and is the lossy step itself: the row optimiser runs at strength 0, where it changes no pixel */
    if (o->have_colors) {
        o->indexed = true;
        if (!o->have_strength) o->strength = 0;
    }
    if (o->indexed || size) o->gpu_deflate = true;
    return SUCCESS;
}

pngloss_error cli_options_check(const struct cli_options *o, FILE *err)
{
    const bool quality = o->search == CLI_SEARCH_QUALITY || o->search == CLI_SEARCH_BOTH;
    const bool size = o->search == CLI_SEARCH_SIZE || o->search == CLI_SEARCH_BOTH;
    if (o->strength > 255) return refuse(err, "Must specify a strength in the range 0-255.\n");
    if (!(o->target_psnr >= 0.0)) return refuse(err, "Must specify a PSNR target of 0 dB or more.\n");
    if (o->have_target_ssim && !(o->target_ssim > 0.0 && o->target_ssim <= 1.0)) return refuse(err, "Must specify an SSIM target above 0 and at most 1.\n");
    if (o->have_max_error && (o->max_error < 1 || o->max_error > 255)) return refuse(err, "Must specify a largest channel error in the range 1-255.\n");
    if (o->search == CLI_SEARCH_BOTH) return refuse(err, "--target-size cannot be combined with --target-psnr, --target-ssim or --max-error.\n");
    if (o->visible && !(o->distortion || o->ssim || quality)) return refuse(err, "--visible needs one of --distortion, --ssim, --target-psnr, --max-error or --target-ssim.\n");
    if (o->visible && size) return refuse(err, "--visible cannot be combined with --target-size.\n");
    if (size && o->size_value < 1) return refuse(err, "Must specify a size target of at least 1 byte or 1 percent.\n");
    if (o->dither && !o->have_colors) return refuse(err, "--dither requires --colors.\n");
    if (o->have_colors && (o->colors < 2 || o->colors > 256)) return refuse(err, "Must specify a number of colours in the range 2-256.\n");
    if (o->have_colors && o->strength != 0) return refuse(err, "--colors cannot be combined with a strength above 0: the palette is the lossy step.\n");
    if (o->have_colors && (o->search != CLI_SEARCH_NONE || o->ssim || o->visible))
        return refuse(err, "--colors cannot be combined with --target-size, --target-psnr, --target-ssim, --max-error, --ssim or --visible.\n");
    if (o->indexed && o->search != CLI_SEARCH_NONE) return refuse(err, "--indexed cannot be combined with --target-size, --target-psnr, --target-ssim or --max-error.\n");
    if (o->bleed < 1 || o->bleed > 32767) return refuse(err, "Must specify a bleed divider in the range 1-32767.\n");
    if (o->extension && o->output_path) return refuse(err, "--ext and --output options can't be used at the same time\n");
    if (o->output_path && o->num_files != 1)
        return refuse(err, "  error: Only one input file is allowed when --output is used. This error also happens when filenames with spaces are not in quotes.\n");
    if (o->to_stdout && !o->from_stdin && o->num_files != 1)
        return refuse(err, "  error: Only one input file is allowed when using the special output path \"-\" to write to stdout. This error also happens when filenames with spaces are not in quotes.\n");
    if (!o->num_files && !o->from_stdin) {
        fputs("No input files specified.\n", err);
        return MISSING_ARGUMENT;
    }
    /* the colour-count search of --colors: behind every older rule, so that what those answer stays what it was */
    if (o->have_colors_psnr && !o->have_colors) return refuse(err, "--colors-psnr requires --colors.\n");
    if (o->have_colors_max_error && !o->have_colors) return refuse(err, "--colors-max-error requires --colors.\n");
    if (o->have_colors_psnr && !o->colors_psnr_ok) return refuse(err, "--colors-psnr requires a numeric argument\n");
    if (o->have_colors_psnr && !(o->colors_psnr > 0.0)) return refuse(err, "Must specify a colour PSNR target above 0 dB.\n");
    if (o->have_colors_max_error && !o->colors_max_error_ok) return refuse(err, "--colors-max-error requires a numeric argument\n");
    if (o->have_colors_max_error && (o->colors_max_error < 1 || o->colors_max_error > 255))
        return refuse(err, "Must specify a largest colour channel error in the range 1-255.\n");
    /* the space of --colors: behind those again */
    if (o->colors_visible && !o->have_colors) return refuse(err, "--colors-visible requires --colors.\n");
    /* the bit depth of the palette files: behind those again (--colors implies --indexed) */
    if (o->have_index_depth && !o->indexed) return refuse(err, "--index-depth requires --indexed or --colors.\n");
    if (o->have_index_depth && !o->index_depth_ok) return refuse(err, "--index-depth requires auto, min or 8\n");
    return SUCCESS;
}

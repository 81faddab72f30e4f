/* cli_report.c -- the lines about one written file (cli_report.h). */
#include "cli_report.h"

#include <stdio.h>

unsigned cli_stored_channel_mask(unsigned bytes_per_pixel)
{
    return bytes_per_pixel == 1 ? 0x2u : bytes_per_pixel == 2 ? 0xAu : bytes_per_pixel == 3 ? 0x7u : 0xFu;
}

void cli_report_distortion(char *line, size_t cap, const pngloss_hip_distortion *d, unsigned bytes_per_pixel, bool visible)
{
    if (!d->changed_pixels && visible) { snprintf(line, cap, "  distortion (visible): none, %llu visible pixels\n", (unsigned long long)d->pixels); return; }
    if (!d->changed_pixels) { snprintf(line, cap, "  distortion: none (lossless)\n"); return; }
    const unsigned mask = cli_stored_channel_mask(bytes_per_pixel);
    unsigned largest = 0;
    for (int c = 0; c < 4; c++)
        if ((mask >> c & 1u) && d->max_abs[c] > largest) largest = d->max_abs[c];
    snprintf(line, cap, visible ? "  distortion (visible): PSNR %.2f dB, %llu of %llu visible pixels changed, largest channel error %u\n"
                                : "  distortion: PSNR %.2f dB, %llu of %llu pixels changed, largest channel error %u\n", pngloss_hip_psnr_db(d, mask),
             (unsigned long long)d->changed_pixels, (unsigned long long)d->pixels, largest);
}

void cli_report_ssim(char *line, size_t cap, const pngloss_hip_ssim *r, enum cli_search search, unsigned bytes_per_pixel, bool visible)
{
    if (!r) {
        snprintf(line, cap, "%s", search == CLI_SEARCH_SIZE ? "  ssim: not measured (the size search keeps no SSIM record)\n"
                                : search == CLI_SEARCH_QUALITY ? "  ssim: not measured (a strength search measures it only with --target-ssim)\n" : "");
        return;
    }
    if (!r->windows) { snprintf(line, cap, "%s", visible ? "  ssim (visible): not measured (no 8x8 window with a visible pixel)\n" : "  ssim: not measured (smaller than one 8x8 window)\n"); return; }
    const unsigned mask = cli_stored_channel_mask(bytes_per_pixel);
    int32_t worst = 65536;
    for (int c = 0; c < 4; c++)
        if ((mask >> c & 1u) && r->min_q16[c] < worst) worst = r->min_q16[c];
    snprintf(line, cap, visible ? "  ssim (visible): mean %.4f, worst window %.4f, %llu windows with visible pixels\n" : "  ssim: mean %.4f, worst window %.4f, %llu windows\n",
             pngloss_hip_ssim_mean(r, mask), (double)worst / 65536.0, (unsigned long long)r->windows);
}

void cli_report_strength(char *line, size_t cap, unsigned strength, unsigned probes)
{
    snprintf(line, cap, "  strength %u chosen in %u probes\n", strength, probes);
}

void cli_report_indexed(char *line, size_t cap, const pngloss_hip_palette *p)
{
    snprintf(line, cap, "  indexed: %u colours, %llu bytes of image data and %llu of palette against %llu bytes as truecolour\n", p->colors,
             (unsigned long long)p->indexed_bytes, (unsigned long long)(12u + 3u * p->entries + (p->trns_entries ? 12u + p->trns_entries : 0u)),
             (unsigned long long)p->truecolor_bytes);
}

void cli_report_index_depth(char *line, size_t cap, const pngloss_hip_index_depth *r)
{
    if (r->bit_depth < 1 || r->bit_depth >= 8) { if (cap) line[0] = 0; return; }
    if (r->indexed8_bytes)
        snprintf(line, cap, "  index depth: %u bits, %llu bytes of packed image data against %llu bytes at 8 bits\n", r->bit_depth,
                 (unsigned long long)r->packed_bytes, (unsigned long long)r->indexed8_bytes);
    else
        snprintf(line, cap, "  index depth: %u bits, %llu bytes of packed image data (the 8-bit stream was not written)\n", r->bit_depth,
                 (unsigned long long)r->packed_bytes);
}

void cli_report_quant(char *line, size_t cap, const pngloss_hip_quant_report *q)
{
    char in[32];
    if (q->colors_in > 256) snprintf(in, sizeof in, "more than 256");
    else snprintf(in, sizeof in, "%u", q->colors_in);
    snprintf(line, cap, "  colors: %s in the input, %u palette entries%s\n", in, q->entries, q->exact ? ", exact (no pixel changed)" : "");
}

void cli_report_chosen_colors(char *line, size_t cap, const pngloss_hip_quant_target_report *r, unsigned max_colors)
{
    if (!r->reached) {
        snprintf(line, cap, "  chosen: %u of at most %u colours, target not reached\n", r->colors, max_colors);
        return;
    }
    char psnr[32];
    if (!r->probe_distortion.changed_pixels) snprintf(psnr, sizeof psnr, "exact");
    else snprintf(psnr, sizeof psnr, "%.2f dB", pngloss_hip_psnr_db(&r->probe_distortion, 0xFu));
    snprintf(line, cap, "  chosen: %u of at most %u colours, %s (%u probes)\n", r->colors, max_colors, psnr, r->probes);
}

void cli_report_colors_missed(char *line, size_t cap, const char *name, unsigned max_colors)
{
    snprintf(line, cap, "  warning: %s: the colour target is not reached with %u colours; written at %u colours\n", name, max_colors, max_colors);
}

void cli_report_dither(char *line, size_t cap, const pngloss_hip_quant_report *q)
{
    snprintf(line, cap, "%s", q->exact ? "" : "  dither: Floyd-Steinberg\n");
}

void cli_report_colors_space(char *line, size_t cap, const pngloss_hip_quant_report *q)
{
    snprintf(line, cap, "%s", q->exact ? "" : "  colour space: premultiplied\n");
}

void cli_report_budget_missed(char *line, size_t cap, const char *name, size_t budget, size_t written, unsigned strength)
{
    snprintf(line, cap, "  warning: %s: budget of %zu bytes not reached, wrote %zu bytes at strength %u\n", name, budget, written, strength);
}

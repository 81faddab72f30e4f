/* cli_report.h -- the lines the pngloss tool prints about one written file, formatted from the library's plain records into the caller's buffer
 * (each ends in a newline; a line that does not fit is cut, as every message of the tool is).  tests/c/cli_report_host.c compares them with the
 * Python mirrors of the GPU tests on the CPU. */
#ifndef PNGLOSS_AMD_CLI_REPORT_H
#define PNGLOSS_AMD_CLI_REPORT_H

#include <stdbool.h>
#include <stddef.h>

#include "../../include/pngloss_hip.h"
#include "../../include/pngloss_hip_indexed.h"
#include "../../include/pngloss_hip_index_depth.h"
#include "../../include/pngloss_hip_quant.h"
#include "../../include/pngloss_hip_dither.h"
#include "../../include/pngloss_hip_quant_target.h"
#include "cli_options.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the channels a result of bytes_per_pixel 1, 2, 3, 4 stores, as pngloss_hip_psnr_db and pngloss_hip_ssim_mean take them (gray is the G channel) */
unsigned cli_stored_channel_mask(unsigned bytes_per_pixel);

/* --distortion.  visible: the record is over premultiplied channels and `pixels` counts the visible ones */
void cli_report_distortion(char *line, size_t cap, const pngloss_hip_distortion *d, unsigned bytes_per_pixel, bool visible);

/* --ssim: mean and worst window over the stored channels.  r == NULL: the file has no record; the line then says why the search kept none, and
 * is empty where there was no search */
void cli_report_ssim(char *line, size_t cap, const pngloss_hip_ssim *r, enum cli_search search, unsigned bytes_per_pixel, bool visible);

/* -v: what a search chose; what --indexed decided; and the warning of a --target-size budget that -s did not reach */
void cli_report_strength(char *line, size_t cap, unsigned strength, unsigned probes);
void cli_report_indexed(char *line, size_t cap, const pngloss_hip_palette *p);
/* ... with --index-depth, the line behind it for a file kept below 8 bits: the depth, the packed stream's size and the 8-bit stream's (which
 * --index-depth min does not write); empty for any other file */
void cli_report_index_depth(char *line, size_t cap, const pngloss_hip_index_depth *r);
/* -v with --colors: the input's colours, the palette entries of what is written, and whether the image was left as it was */
void cli_report_quant(char *line, size_t cap, const pngloss_hip_quant_report *q);
/* ... with --colors-psnr / --colors-max-error, the line behind it: the colour count the search chose below --colors M, the PSNR over all four
 * channels of the probe it ended on and the probes taken -- or that even M colours did not reach the target */
void cli_report_chosen_colors(char *line, size_t cap, const pngloss_hip_quant_target_report *r, unsigned max_colors);
/* the warning for a file whose colour target --colors M did not reach: it was written at M colours */
void cli_report_colors_missed(char *line, size_t cap, const char *name, unsigned max_colors);
/* ... with --dither, the line behind it: empty for a file that was exact, which is never dithered */
void cli_report_dither(char *line, size_t cap, const pngloss_hip_quant_report *q);
/* ... with --colors-visible, the line behind those: empty for a file that was exact, which no space touches */
void cli_report_colors_space(char *line, size_t cap, const pngloss_hip_quant_report *q);
void cli_report_budget_missed(char *line, size_t cap, const char *name, size_t budget, size_t written, unsigned strength);

#ifdef __cplusplus
}
#endif
#endif

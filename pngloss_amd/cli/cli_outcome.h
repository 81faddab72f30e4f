/* cli_outcome.h -- what an answer of the device library means for ONE file of the pngloss tool.  Small pure functions, each with a single caller
 * in pngloss_main.c; a slip in one of them writes an unoptimised or a garbage file without a word, so tests/c/cli_outcome_host.c runs them over
 * their whole domain on the CPU. */
#ifndef PNGLOSS_AMD_CLI_OUTCOME_H
#define PNGLOSS_AMD_CLI_OUTCOME_H

#include <stdbool.h>
#include <stddef.h>

#include "../../include/pngloss_hip.h"
#include "cli_options.h"

/* The file's status after the optimise call, from the call's return code and results[k].status: 0, or the code the file fails with.
 * A batch in which single images failed returns PNGLOSS_INTERNAL_ABORT and leaves the others done.  Unlike the reference (pngloss.c:266 ignores
 * the return value) a failed optimisation is an error: there is no CPU path to fall back to, and writing an unoptimised file silently would be
 * wrong. */
static inline int cli_status_after_optimise(int batch_rc, int image_status)
{
    if (batch_rc == PNGLOSS_SUCCESS || (batch_rc == PNGLOSS_INTERNAL_ABORT && image_status == 0)) return PNGLOSS_SUCCESS;
    return batch_rc;
}

/* a search call that returned this code has filled its reports */
static inline bool cli_reports_filled(int batch_rc) { return batch_rc == PNGLOSS_SUCCESS || batch_rc == PNGLOSS_INTERNAL_ABORT; }

/* Whether the file has a distortion / SSIM / palette record.  `asked`: the switch (--distortion, --ssim, --indexed) is on.  A search returns the
 * records in its reports; the plain call keeps them in the context, and last_ok says that pngloss_hip_multi_last_* gave this file's.  The size
 * search keeps no SSIM record, the quality search one only with --target-ssim, and neither search writes indexed streams. */
static inline bool cli_have_distortion(enum cli_search search, bool asked, int batch_rc, bool last_ok)
{
    return asked && (search == CLI_SEARCH_NONE ? last_ok : cli_reports_filled(batch_rc));
}

static inline bool cli_have_ssim(enum cli_search search, bool asked, bool have_target_ssim, int batch_rc, bool last_ok)
{
    if (search == CLI_SEARCH_NONE) return asked && last_ok;
    return search == CLI_SEARCH_QUALITY && asked && have_target_ssim && cli_reports_filled(batch_rc);
}

static inline bool cli_have_palette(enum cli_search search, bool asked, bool last_ok)
{
    return search == CLI_SEARCH_NONE && asked && last_ok;
}

/* an indexed stream that came without its palette cannot be written (a failed call is reported by cli_status_after_optimise instead) */
static inline bool cli_indexed_without_palette(int color_type, bool have_palette, int batch_rc)
{
    return color_type == 3 && !have_palette && batch_rc == PNGLOSS_SUCCESS;
}

/* The file's status after the device read (--gpu-read): 0, or the code it fails with.  setup_rc: what preparing the batch gave; batch_rc: the
 * decode call's return code; st: this file's own status; explained: some file's status is non-zero.
 * A failure of the batch as a whole arrives in every file's status (pngloss_hip.h); a return code that no status explains is treated the same
 * way -- never take a file for decoded on the strength of st == 0 alone. */
static inline int cli_status_after_device_read(int setup_rc, int batch_rc, int st, bool explained)
{
    if (setup_rc != PNGLOSS_SUCCESS) return setup_rc;
    if (st) return st;
    return batch_rc != PNGLOSS_SUCCESS && !explained ? batch_rc : PNGLOSS_SUCCESS;
}

/* --target-size: the budget of one written file in bytes, from N bytes or P percent of the input file's size; at least 1 */
static inline size_t cli_file_budget(bool percent, unsigned long long value, size_t input_file_size)
{
    const unsigned long long want = percent ? (unsigned long long)((long double)input_file_size * (long double)value / 100.0L) : value;
    return want < 1 ? 1 : (size_t)want;
}

/* ... and the budget of its zlib stream, from the largest stream that the file's container leaves room for (png_stream_largest_stream).  A
 * budget below the container alone can never be met: the library gets 1 byte, which writes the file at -s */
static inline uint64_t cli_stream_budget(size_t largest_stream) { return largest_stream ? largest_stream : 1; }

#endif

/*
 * pngloss_hip.h -- C ABI of the MI355X (gfx950) implementation of pngloss's filter+quantise hot path.
 *
 * libpngloss_hip.so is a drop-in for the ONE seam the reference has on this path:
 *
 *     pngloss_file_internal()  --calls-->  optimize_with_rows()        /root/reference/src/pngloss.c:266
 *                                                                      /root/reference/src/pngloss_image.h:21-25
 *
 * Section 1 re-exports that seam (and its two legacy siblings) with the reference's exact names, argument meaning,
 * ownership rules and return codes, so that relinking pngloss.c against this library instead of
 * pngloss_image.c/optimize_state.c/color_delta.c changes nothing but the speed.  Section 2 is the device-resident /
 * batched extension the reference does not have (its per-file loop, pngloss.c:173, is sequential).
 *
 * Plain C, plain pointers and sizes; no HIP or torch types appear in any signature (streams are passed as void*).
 * There is NO CPU fallback behind these entry points: if the HIP runtime, a gfx950 device or the kernels are
 * unavailable they fail loudly (message on stderr + PNGLOSS_HIP_ERROR), they never silently compute on the host.
 */
#ifndef PNGLOSS_HIP_H
#define PNGLOSS_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes: the subset of the reference's pngloss_error (rwpng.h:23-38) this path can produce ---------- */
#ifndef PNGLOSS_ERROR_CODES
#define PNGLOSS_ERROR_CODES
#define PNGLOSS_SUCCESS             0   /* SUCCESS              rwpng.h:24 */
#define PNGLOSS_OUT_OF_MEMORY_ERROR 17  /* OUT_OF_MEMORY_ERROR  rwpng.h:30 (host or device allocation failed) */
#define PNGLOSS_INVALID_ARGUMENT    4   /* INVALID_ARGUMENT     rwpng.h:27 (bleed outside 1..32767 etc.; the CLI
                                           validates this at pngloss.c:123-131, the library re-checks) */
#define PNGLOSS_HIP_ERROR           64  /* new: HIP runtime / device / kernel failure (no reference equivalent) */
#define PNGLOSS_INTERNAL_ABORT      65  /* new: the invariant the reference abort()s on (optimize_state.c:216-219,
                                           245-248; pngloss_image.c:268-271) was violated on the device */
#endif

/* =====================================================================================================
 * 1. Drop-in seam (host pointers).  Replaces /root/reference/src/pngloss_image.h:14-29.
 * ===================================================================================================== */

/* pngloss_image.h:7-11 -- packed image with 1..4 bytes per pixel, rows need not be contiguous. */
typedef struct {
    unsigned char **rows;
    uint32_t width, height;
    uint_fast8_t bytes_per_pixel;
} pngloss_image;

/* Replaces optimize_with_rows(), pngloss_image.h:21-25 / pngloss_image.c:52-156.
 *   rows          height pointers to width*4 bytes of RGBA8 each, caller-owned, rewritten IN PLACE
 *   row_filters   caller-allocated height bytes or NULL.  Non-NULL: receives libpng filter FLAG values
 *                 0x08,0x10,0x20,0x40,0x80 (PNG_FILTER_NONE..PAETH, pngloss_image.c:290-306) and only row 0 is
 *                 forced to libpng's heuristic filter.  NULL: every row is (pngloss_image.c:210), no IDs returned.
 *   verbose       prints the progress display of pngloss_image.c:214-237 (spinner + percentage of finished rows at 10 Hz, fed
 *                 by a host-mapped word the engine writes per row), then "compression complete" / "used N unique symbols"
 *                 to stderr like :309-325
 *   quantization_strength 0..255, bleed_divider 1..32767 (pngloss.c:123-131)
 * Returns PNGLOSS_SUCCESS or an error above.  Output bytes and filter IDs are bit-identical to the reference. */
int optimize_with_rows(unsigned char **rows, uint32_t width, uint32_t height, unsigned char *row_filters,
                       bool verbose, uint_fast8_t quantization_strength, int_fast16_t bleed_divider);

/* Replaces optimize_with_stride(), pngloss_image.h:17-20 / pngloss_image.c:40-50 (row_filters = NULL mode). */
void optimize_with_stride(unsigned char *pixels, uint32_t width, uint32_t height, uint32_t stride,
                          bool verbose, uint_fast8_t quantization_strength, int_fast16_t bleed_divider);

/* Replaces optimizeForAverageFilter(), pngloss_image.h:14-16 / pngloss_image.c:29-38 (RGBA, bleed fixed at 2). */
void optimizeForAverageFilter(unsigned char pixels[], int width, int height, int quantization);

/* Replaces optimize_image(), pngloss_image.h:26-29 / pngloss_image.c:159-333: the lower seam on an already packed
 * 1/2/3/4 bytes-per-pixel image (no gray/alpha detection). */
int optimize_image(pngloss_image *image, unsigned char *row_filters, bool verbose,
                   uint_fast8_t quantization_strength, int_fast16_t bleed_divider);

/* =====================================================================================================
 * 2. Device-resident, batched extension (new; the natural batching point is pngloss.c:173).
 * ===================================================================================================== */

typedef struct pngloss_hip_ctx pngloss_hip_ctx;

/* One RGBA8 image resident in device memory. */
typedef struct {
    void    *d_rgba;         /* device pointer, width*height*4 bytes, rows contiguous; rewritten in place       */
    void    *d_row_filters;  /* device pointer to height bytes, or NULL (=> all rows adaptive, no IDs)           */
    uint32_t width, height;
} pngloss_hip_image_desc;

/* Per-image result record (host memory, filled after the stream has been synchronised by _finish). */
typedef struct {
    int32_t  status;            /* PNGLOSS_SUCCESS / PNGLOSS_INTERNAL_ABORT                                        */
    uint32_t bytes_per_pixel;   /* 1 gray, 2 gray+alpha, 3 rgb, 4 rgba -- what pngloss_image.c:64-96 detects       */
    uint32_t unique_symbols;    /* non-zero bins of the final histogram (pngloss_image.c:311-325)                  */
    uint32_t retried_rows;      /* rows that needed the strength-decrement retry (pngloss_image.c:266-274)         */
    uint32_t repaired_pixels;   /* diagnostics, no reference equivalent: segment engine: validation restarts (epochs); workgroup engine:
                                   pixels its first chain wave redid exactly                          */
} pngloss_hip_result;

/* Number of HIP devices visible, or a negative PNGLOSS_HIP_ERROR-style code if the runtime is unusable. */
int pngloss_hip_device_count(void);

/* Create / destroy a context bound to one device (device < 0: the current device).  NULL on failure. */
pngloss_hip_ctx *pngloss_hip_create(int device);
void pngloss_hip_destroy(pngloss_hip_ctx *ctx);

/* Enqueue the whole hot path for n device-resident images on `stream` (a hipStream_t passed as void*, NULL = the
 * default stream).  Images are independent and run concurrently.
 * Asynchronous: returns without waiting for the device; call pngloss_hip_finish() to synchronise and collect results.
 * Work the caller enqueues on `stream` behind this call runs behind the batch.  (Two row engines, chosen per batch: one
 * workgroup per image -- everything is enqueued on `stream` before the call returns; one image spread over the whole device -- the
 * number of row attempts depends on the data, so a helper thread of the context feeds them to a stream of the context's own and
 * `stream` waits for the device-written "images finished" word (hipStreamWaitValue32).  On a device without stream memory operations
 * the call waits for that thread instead: then, and only then, it blocks for the duration of the row engine.)
 * One batch per context at a time: the next call must follow pngloss_hip_finish(). */
int pngloss_hip_optimize_batch_async(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                     unsigned quantization_strength, long bleed_divider, void *stream);

/* Wait for the last enqueued batch, copy back its n result records (results may be NULL). */
int pngloss_hip_finish(pngloss_hip_ctx *ctx, pngloss_hip_result *results, size_t n);

/* The synchronous form: enqueue + finish in one call.  Its caller waits on the host anyway, so `stream` gets no device-side wait for the segment engine's "finished"
 * word (the helper thread is joined inside the call and `stream` is ordered behind the engine's streams by an event): the engine runs 1-7 % faster without a queue
 * polling that word, and batches of twelve and more frames run as three launch sequences instead of two.  Results are the same either way. */
int pngloss_hip_optimize_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                               unsigned quantization_strength, long bleed_divider, void *stream,
                               pngloss_hip_result *results);

/* The same for images in HOST memory (the batch form of optimize_with_rows: this is what a multi-file CLI loop calls
 * instead of pngloss.c:173-208's one-file-at-a-time loop).  rgba: width*height*4 contiguous bytes, rewritten in place;
 * row_filters: height bytes or NULL.  Uploads, runs one batch, downloads; synchronous. */
typedef struct {
    unsigned char *rgba;
    unsigned char *row_filters;
    uint32_t width, height;
} pngloss_hip_host_image;

int pngloss_hip_optimize_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                    unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results);

/* ---- Every GPU of the node.  The reference's command line walks its files one at a time (/root/reference/src/pngloss.c:
 * 173-208); a node with several GPUs deals them out instead: one context per device, images split by size (longest first
 * to the least loaded device), one host thread per context, no collective -- images are independent.
 * devices: NULL/"" = $PNGLOSS_DEVICES if set, else every visible device; otherwise a comma separated list of device ordinals,
 * which may repeat ("0,0" = two contexts sharing device 0: the split logic without a second GPU). */
typedef struct pngloss_hip_multi pngloss_hip_multi;
pngloss_hip_multi *pngloss_hip_multi_create(const char *devices);
void pngloss_hip_multi_destroy(pngloss_hip_multi *multi);
int pngloss_hip_multi_count(const pngloss_hip_multi *multi);
/* owner[i] = index of the context image i goes to (deterministic LPT split; exported so that callers can plan and tests can
 * check it against pngloss_amd/shard.py) */
void pngloss_hip_multi_split(const pngloss_hip_host_image *images, size_t n, int parts, int *owner);

/* As above, and additionally returns, per image, the FILTERED SCANLINES a PNG encoder deflates -- the first piece of
 * the PNG write side done on the device (replaces libpng's png_write_row filtering inside rwpng_write_image24,
 * /root/reference/src/rwpng.c:477-501,558-609): the colour type is re-detected from the optimised pixels, gray images
 * are repacked, row 0 (every row when row_filters is NULL) takes libpng's heuristic filter, the others the filter the
 * optimiser chose.  The host then only deflates and frames chunks (pngloss_amd/cli/png_stream_writer.c).
 *   filter_types  caller-allocated height bytes, receives the PNG filter type 0..4 of every scanline
 *   scanlines     caller-allocated height*pitch bytes, receives width*channels filtered bytes per row
 *   pitch         in: bytes between rows of `scanlines`, >= width*4
 *   color_type    out: 0 gray, 4 gray+alpha, 2 RGB, 6 RGBA (8 bits per sample)
 * Entries whose buffers are NULL are skipped. */
typedef struct {
    unsigned char *filter_types;
    unsigned char *scanlines;
    size_t pitch;
    int color_type;
} pngloss_hip_scanlines;

int pngloss_hip_optimize_batch_host_emit(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                         unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                         pngloss_hip_scanlines *scanlines);

/* Same again, but the device also DEFLATES the scanlines: per image the caller gets the complete zlib stream of the
 * PNG's IDAT data (what /root/reference/src/rwpng.c:477-637 obtains from libpng + zlib level 9 on the CPU, and where
 * the reference tool spends its time once the hot path is fast).  The stream inflates to exactly the scanlines the
 * _emit call returns -- so the decoded PNG is identical -- but it is not the byte sequence zlib would write:
 * the encoder is the GPU one of pngloss_amd/csrc/pl_deflate_core.h (multi-level match search, optimal parse, 256 KiB
 * blocks that each end byte-aligned).  On the files of the reference's suite its output is 6-10 % smaller than zlib
 * level 9 / Z_FILTERED.
 * `data` must have room for pngloss_hip_zlib_bound(width, height) bytes; `size` = 0 for an empty image.  One image may
 * have at most 1 GiB of scanlines ((4*width+1)*height; positions are 32-bit on the device): larger ones make the call
 * return PNGLOSS_INVALID_ARGUMENT -- use the _emit form and a CPU deflate for those. */
typedef struct {
    unsigned char *data;      /* in: caller's buffer; out: zlib stream (header 78 DA ... Adler-32) */
    size_t capacity;          /* in */
    size_t size;              /* out */
    int color_type;           /* out: 0, 2, 4 or 6; with the option "indexed" on also 3 (pngloss_hip_indexed.h: pngloss_hip_last_palette has the palette) */
    uint32_t blocks[3];       /* out: deflate blocks written as stored / fixed / dynamic */
    uint32_t flags;           /* in: PNGLOSS_HIP_Z_* */
} pngloss_hip_zstream;

/* the caller only wants the stream: the optimised pixels (and row_filters) are not copied back to the host image */
#define PNGLOSS_HIP_Z_STREAM_ONLY 1u

size_t pngloss_hip_zlib_bound(uint32_t width, uint32_t height);

/* pngloss_hip_optimize_batch_host / _emit / _zlib over every context of `multi`: scanlines and streams may be NULL
 * (independently); results[], scanlines[], streams[] are indexed like images[].  Returns the worst status; a batch in which
 * single images failed (results[i].status != 0) returns PNGLOSS_INTERNAL_ABORT with every other image done. */
int pngloss_hip_multi_optimize_batch_host(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                          unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                          pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams);

int pngloss_hip_optimize_batch_host_zlib(pngloss_hip_ctx *ctx, const pngloss_hip_host_image *images, size_t n,
                                         unsigned quantization_strength, long bleed_divider, pngloss_hip_result *results,
                                         pngloss_hip_zstream *streams);

/* Milliseconds the last _zlib call spent in the deflate stage (device work + the block-size round trip). */
double pngloss_hip_last_deflate_ms(const pngloss_hip_ctx *ctx);

/* Duration in milliseconds of the row-engine kernel of the last finished batch, measured with hipEvents recorded
 * on the launch stream immediately around that kernel (what bench.py's roofline block reports).  < 0 if none. */
double pngloss_hip_last_engine_ms(const pngloss_hip_ctx *ctx);
/* Same for the whole enqueued pipeline (classify + histograms + repack + engine + unpack). */
double pngloss_hip_last_total_ms(const pngloss_hip_ctx *ctx);

/* Final 256-bin symbol histogram of image `index` of the last finished batch (host buffer of 256 uint32). */
int pngloss_hip_last_histogram(pngloss_hip_ctx *ctx, size_t index, uint32_t *hist256);

/* The tables the row engines break ties with (optimize_state.c:228-231), of image `index` of the last finished batch, as the device holds them:
 * freq[f * 256 + s] is the reference's original_frequency[f][s] (f = none, sub, up, average, paeth) over the image in its byte-per-pixel class,
 * rank[f * 256 + s] the number of s' with freq[f][s'] < freq[f][s].  Host buffers of 5 * 256 uint32 each; either may be NULL, not both.  Refused
 * (PNGLOSS_INVALID_ARGUMENT) where pngloss_hip_last_histogram is: while a batch is pending, for an index out of range, after a target or size
 * search; the index follows the chunks of a host window in the same way.  The row-statistics engine (strength 0) keeps no ranks: asking for `rank`
 * of an image it took is refused as well.  For tests and diagnosis: two copies from the device, nothing on the path of a batch. */
int pngloss_hip_last_original_tables(pngloss_hip_ctx *ctx, size_t index, uint32_t *freq, uint32_t *rank);   /* [5][256] each; either may be NULL, not both */

/* ---- How lossy a run was, measured on the device (no reference equivalent: the reference tool reports file sizes only).  The optimiser works in
 * place, so the original is gone before a caller could compare -- and on the fast paths (device-resident batches, frames handed over by
 * pngloss_hip_png_decode_batch_device[_z], PNGLOSS_HIP_Z_STREAM_ONLY) original and result never exist side by side on the host.  With the option
 * "distortion" at "on" (pngloss_hip_set_option) every batch that goes through pngloss_hip_optimize_batch[_async], _batch_host, _host_emit or
 * _host_zlib keeps a copy of its originals in an arena of the context (one more width * height * 4 bytes per image; if that cannot be had the
 * call returns PNGLOSS_OUT_OF_MEMORY_ERROR before anything is enqueued) and compares the final RGBA8 with it: one copy kernel in front of the
 * pipeline and one measuring kernel behind it, both on the caller's stream and inside the window pngloss_hip_last_total_ms reports.  Pixels,
 * filter IDs, scanlines and zlib streams do not depend on the option.  The section-1 seam has no context to ask and is never measured.
 *
 * The record of an RGBA8 pair (a = original, b = result; channel c = 0..3 is R, G, B, A).  All integers: exact, and independent of the order of
 * summation. */
typedef struct {
    uint64_t pixels;            /* width * height                                                                  */
    uint64_t changed_pixels;    /* pixels in which any channel differs                                             */
    uint64_t sq_err[4];         /* per channel: sum of (b_c - a_c)^2                                               */
    uint32_t max_abs[4];        /* per channel: max of |b_c - a_c|                                                 */
} pngloss_hip_distortion;

/* Record of image `index` of the last finished batch.  PNGLOSS_INVALID_ARGUMENT when that batch ran with the option off, when the index is out of
 * range or while a batch is pending.  After a host window that ran in chunks the index follows the chunks, as for pngloss_hip_last_histogram.
 * The record of an image whose status != 0 is unspecified. */
int pngloss_hip_last_distortion(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_distortion *out);

/* The same measurement on its own: n pairs of device-resident RGBA8 images (width * height * 4 contiguous bytes each, any alignment of 4), one
 * launch of the same kernel, out[i] = record of pair i.  Synchronous: enqueued on `stream` (NULL = the default stream) and waited for.  A pair
 * without pixels gives an all-zero record.  Compares the outputs of two builds or settings; independent of the option above.  Not while a batch
 * is in flight on the context (PNGLOSS_INVALID_ARGUMENT). */
typedef struct {
    const void *d_a, *d_b;
    uint32_t width, height;
} pngloss_hip_image_pair;

int pngloss_hip_compare_batch(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out, void *stream);

/* Peak signal-to-noise ratio in dB over the channels of `channel_mask` (bit c = channel c):
 *     10 * log10(255^2 * pixels * popcount(mask) / sum over the mask's channels of sq_err[c])
 * +INFINITY when that sum is 0; NaN for pixels == 0, for mask 0 and for a mask above 0xF.  Host arithmetic only: needs no device.
 * (For an image the optimiser reports as bytes_per_pixel 1, 2, 3, 4 the channels that are stored are 0x2, 0xA, 0x7, 0xF.) */
double pngloss_hip_psnr_db(const pngloss_hip_distortion *d, unsigned channel_mask);

/* pngloss_hip_set_option on every context of `multi` (the worst return code), and the record of images[index] of the last
 * pngloss_hip_multi_optimize_batch_host call, whichever context it went to. */
int pngloss_hip_multi_set_option(pngloss_hip_multi *multi, const char *name, const char *value);
int pngloss_hip_multi_last_distortion(pngloss_hip_multi *multi, size_t index, pngloss_hip_distortion *out);

/* ---- Structural similarity (SSIM) per image, measured on the device (no reference equivalent).  PSNR counts every changed sample as loss; the
 * optimiser's error diffusion deliberately trades a larger per-pixel error for a result whose local mean and structure stay put, which is what
 * SSIM measures.  With the option "ssim" at "on" (pngloss_hip_set_option; independent of "distortion") every batch that goes through
 * pngloss_hip_optimize_batch[_async], _batch_host, _host_emit or _host_zlib keeps its originals exactly as for "distortion" -- ONE arena and one copy
 * kernel, whether one of the two options is on or both -- and one more measuring kernel runs behind the pipeline, on the caller's stream and
 * inside the window pngloss_hip_last_total_ms reports.  Pixels, filter IDs, scanlines and zlib streams do not depend on the option.
 *
 * The record of an RGBA8 pair (a = original, b = result; channel c = 0..3 is byte c of each pixel word: R, G, B, A).  All integers: exact, and
 * independent of the order of summation.
 *   Windows: 8 x 8 pixels at a stride of 4 in both directions (the layout x264 and libvpx use): origins (4i, 4j) for every i, j with
 *     4i + 8 <= width and 4j + 8 <= height; nx = width >= 8 ? (width - 8) / 4 + 1 : 0, ny likewise, windows = nx * ny.  An image narrower or
 *     lower than 8 pixels has no windows.
 *   Per window and channel, with the exact sums sa, sb, saa, sbb, sab over its 64 pixels, K1 = 26634 and K2 = 239708 (64^2 (0.01 * 255)^2 and
 *     64^2 (0.03 * 255)^2, rounded):
 *         A1 = 2 sa sb + K1                        B1 = sa sa + sb sb + K1
 *         A2 = 2 (64 sab - sa sb) + K2             B2 = 64 (saa + sbb) - sa sa - sb sb + K2
 *         q  = sign(A1 A2) * floor(|A1 A2| * 65536 / (B1 B2))
 *     q lies in [-65536, 65536] and is 65536 exactly when the two windows are equal. */
typedef struct {
    uint64_t windows;           /* nx * ny                                                                         */
    int64_t  sum_q16[4];        /* per channel: sum of q over all windows                                          */
    int32_t  min_q16[4];        /* per channel: the smallest q -- the worst spot; 65536 when windows == 0          */
    uint64_t reserved;          /* 0                                                                               */
} pngloss_hip_ssim;

/* Record of image `index` of the last finished batch.  The rules of pngloss_hip_last_distortion: PNGLOSS_INVALID_ARGUMENT when that batch ran with
 * the option "ssim" off, when the index is out of range or while a batch is pending; after a host window that ran in chunks the index follows the
 * chunks.  The record of an image whose status != 0 is unspecified. */
int pngloss_hip_last_ssim(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_ssim *out);
int pngloss_hip_multi_last_ssim(pngloss_hip_multi *multi, size_t index, pngloss_hip_ssim *out);

/* The same measurement on its own, as pngloss_hip_compare_batch: n pairs of device-resident RGBA8 images (any alignment of 4), one launch of the
 * same kernel, out[i] = record of pair i.  Synchronous.  A pair without windows gives { 0, { 0, 0, 0, 0 }, { 65536, 65536, 65536, 65536 }, 0 }.
 * Independent of the options; not while a batch is in flight on the context (PNGLOSS_INVALID_ARGUMENT). */
int pngloss_hip_compare_batch_ssim(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_ssim *out, void *stream);

/* Mean SSIM over the channels of `channel_mask` (bit c = channel c), 1.0 for equal images:
 *     (double)(sum over the mask's channels of sum_q16[c]) / (65536.0 * windows * popcount(mask))
 * NaN for a NULL record, for windows == 0, for mask 0 and for a mask above 0xF.  Host arithmetic only: needs no device.  The masks are those of
 * pngloss_hip_psnr_db (0x2, 0xA, 0x7, 0xF for bytes_per_pixel 1, 2, 3, 4). */
double pngloss_hip_ssim_mean(const pngloss_hip_ssim *r, unsigned channel_mask);

/* ---- Measuring over visible pixels (no reference equivalent).  The two records above treat RGBA8 as four equal channels over width * height pixels.
 * A pixel whose alpha is 0 in the original and in the result cannot be seen, yet it counts in the denominators and almost always adds no error: on
 * images with transparent areas PSNR and mean SSIM come out better than what a viewer sees.  The option "measure" at "visible"
 * (pngloss_hip_set_option; "all" is the default and is what is described above) changes what the measuring kernels of "distortion" and "ssim" count
 * and what the target searches below accept or refuse on; it changes no pixel, filter ID, scanline or stream.  Definitions, all integers:
 *   pm(p), the premultiplied pixel: alpha as it is; each of R, G, B becomes the integer nearest to c * A / 255, (c * A + 127) / 255 with floor
 *     division (255 is odd: never a tie; at most 255).
 *   A pixel is VISIBLE when its alpha is non-zero in the original or in the result.
 *   pngloss_hip_distortion in visible mode: pixels = the number of visible pixels; changed_pixels = pixels with pm(a) != pm(b) as words; sq_err[c]
 *     and max_abs[c] taken on pm(a) and pm(b) (channel 3 is plain alpha).  An invisible pixel adds 0 to every sum.
 *   pngloss_hip_ssim in visible mode: the window arithmetic above on pm(a) and pm(b); a window counts only if at least one of its 64 pixels is
 *     visible; windows = the number of counted windows; the others add nothing to sum_q16 and do not lower min_q16.  Without a counted window the
 *     record is { 0, { 0, 0, 0, 0 }, { 65536, 65536, 65536, 65536 }, 0 }.
 * Over a background colour g the composited error of a pixel is e_pm - g * e_A / 255 (e_pm, e_A: the errors of a premultiplied channel and of
 * alpha), so the premultiplied channels and alpha together bound the error over every background.
 * pngloss_hip_psnr_db, pngloss_hip_ssim_mean, the byte-per-pixel masks and the acceptance rule below work on visible-mode records as they are; an
 * image without a visible pixel has pixels == 0: nothing to measure.
 *
 * pngloss_hip_compare_batch_visible: the stand-alone measurement in visible mode, pairs as for pngloss_hip_compare_batch; out_distortion[i] and
 * out_ssim[i] = the visible-mode records of pair i; either output may be NULL (its kernel is then not launched).  Synchronous, independent of the
 * options; not while a batch is in flight on the context (PNGLOSS_INVALID_ARGUMENT). */
int pngloss_hip_compare_batch_visible(pngloss_hip_ctx *ctx, const pngloss_hip_image_pair *pairs, size_t n, pngloss_hip_distortion *out_distortion,
                                      pngloss_hip_ssim *out_ssim, void *stream);

/* ---- Indexed-colour streams: the option "indexed" (pngloss_hip_set_option, below) lets the calls that return zlib streams answer with PNG colour
 * type 3 where that makes the smaller file.  Its definitions, its record pngloss_hip_palette and the accessors pngloss_hip_last_palette /
 * pngloss_hip_multi_last_palette are in pngloss_hip_indexed.h, which includes this header. ---- */

/* ---- A strength per image, found from a distortion target (no reference equivalent: the reference tool takes -s and nothing else).  A strength
 * says nothing about how the result will look, and the right one differs from image to image; the optimiser works in place, so a caller who
 * wanted "at least 38 dB" had to reload the original for every try.  Here the original stays on the device between the probes.
 *
 * A probe of an image at a strength is ACCEPTED when all of these hold, rec being its pngloss_hip_distortion against the original and mask the
 * channels its result stores (0x2 / 0xA / 0x7 / 0xF for bytes_per_pixel 1 / 2 / 3 / 4, as for pngloss_hip_psnr_db above):
 *     its status is 0;
 *     min_psnr_db == 0, or pngloss_hip_psnr_db(&rec, mask) >= min_psnr_db;
 *     max_abs_error == 0, or the largest rec.max_abs[c] over the mask's channels is <= max_abs_error.
 * An image without pixels is accepted.  PSNR is NOT monotone in the strength, so the chosen strength is defined by this procedure, per image, and
 * not as "the largest strength that passes":
 *     1. probe M = max_strength; if it is accepted, the chosen strength is M
 *     2. otherwise lo = 0, hi = M (strength 0 changes no pixel and counts as accepted without a probe)
 *     3. while hi - lo > 1: probe mid = (lo + hi) / 2, rounded down; accepted: lo = mid, otherwise hi = mid
 *     4. the chosen strength is lo
 * At most 1 + ceil(log2 M) probes, 1 for M <= 1.  A probe whose status is not 0 ends that image's search: the image keeps that probe's result and
 * status, and its report names that probe's strength. */
typedef struct {
    double   min_psnr_db;    /* 0 = no PSNR condition; +inf = only lossless results pass; NaN or < 0: PNGLOSS_INVALID_ARGUMENT */
    uint32_t max_abs_error;  /* 0 = no condition; 1..255 = largest allowed channel error; > 255: PNGLOSS_INVALID_ARGUMENT */
    uint32_t max_strength;   /* M, 0..255: the search never goes above it; > 255: PNGLOSS_INVALID_ARGUMENT */
} pngloss_hip_target;

typedef struct {
    uint32_t strength;       /* chosen */
    uint32_t probes;         /* probes of the rule above */
    uint32_t runs;           /* row-engine runs spent on this image */
    uint32_t reserved;
    pngloss_hip_distortion distortion;   /* of the result that was kept */
} pngloss_hip_target_report;

/* The search on n device-resident images.  SYNCHRONOUS.  On return image i holds what pngloss_hip_optimize_batch at reports[i].strength writes,
 * byte for byte: pixels, d_row_filters and results[i] -- whose diagnostics slot repaired_pixels is that of the run that produced it
 * (results and reports may be NULL).  Every round the images still searching are grouped by
 * the strength they probe next and each group runs as one ordinary batch, one group after the other: the plan, the engine choice and the engines
 * are those of pngloss_hip_optimize_batch.  Originals, and per image the best result so far with its row filters, live in a search arena of the
 * context (2 * width * height * 4 + height bytes per image; if it cannot be had the call returns PNGLOSS_OUT_OF_MEMORY_ERROR before any image is
 * touched); one batched copy kernel per round moves them, the measuring kernel of the option "distortion" compares against the search's own
 * originals.  No engine run is repeated: runs == probes, except that an image none of whose probes was accepted (M > 0) gets strength 0 run once
 * at the end: runs == probes + 1.  Any other error code than PNGLOSS_INTERNAL_ABORT (single images failed, the others are done) leaves the images
 * unspecified.
 * After the call pngloss_hip_last_distortion, _last_histogram and _last_engine_info return PNGLOSS_INVALID_ARGUMENT (no single batch exists to
 * index); the option "distortion" is left as the caller set it and plays no part in the search. */
int pngloss_hip_optimize_batch_target(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                      const pngloss_hip_target *target, long bleed_divider, void *stream,
                                      pngloss_hip_result *results, pngloss_hip_target_report *reports);

/* The same for host images over every context of `multi`, for the command line tool: the images are split like pngloss_hip_multi_optimize_batch_host
 * splits them; each context uploads its images, finds their strengths with the search above (on copies: nothing is written back), then runs the
 * existing host-window path once per distinct chosen strength on that strength's images -- scanlines, GPU deflate, windows in chunks and
 * PNGLOSS_HIP_Z_STREAM_ONLY as there.  Outputs equal those of pngloss_hip_multi_optimize_batch_host at reports[i].strength, image by image.  This
 * form may spend one more run per image: runs <= probes + 1.  results, scanlines, streams, reports may be NULL (independently).  After the call
 * pngloss_hip_multi_last_distortion returns PNGLOSS_INVALID_ARGUMENT: the records are in the reports. */
int pngloss_hip_multi_optimize_batch_host_target(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                                 const pngloss_hip_target *target, long bleed_divider, pngloss_hip_result *results,
                                                 pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                                 pngloss_hip_target_report *reports);

/* ---- The same search with an SSIM condition.  pngloss_hip_target has no room left, so the target grows into a second struct; the two entry points
 * above forward here with min_ssim = 0 and behave byte for byte as before (the SSIM kernel is not launched for them).
 * A probe is ACCEPTED when the three conditions above hold and
 *     min_ssim == 0, or the probe's pngloss_hip_ssim has no windows, or pngloss_hip_ssim_mean(&ssim, mask) >= min_ssim
 * with the same mask.  An image too small for one 8 x 8 window cannot be measured, so the SSIM condition does not apply to it (the others do).
 * SSIM is no more monotone in the strength than PSNR is: the result is defined by the procedure above, which is unchanged.  With min_ssim != 0
 * every round has one more batched launch: the SSIM kernel on the probed images against the search's own originals. */
typedef struct {
    double   min_psnr_db;    /* as in pngloss_hip_target */
    uint32_t max_abs_error;  /* as in pngloss_hip_target */
    uint32_t max_strength;   /* as in pngloss_hip_target */
    double   min_ssim;       /* 0 = no SSIM condition; 0 < min_ssim <= 1: the smallest allowed mean SSIM over the stored channels; NaN, < 0 or > 1:
                                PNGLOSS_INVALID_ARGUMENT */
} pngloss_hip_target2;

/* pngloss_hip_optimize_batch_target / pngloss_hip_multi_optimize_batch_host_target with a pngloss_hip_target2 and one more argument: ssim, n records
 * of the results that were kept, indexed like images[]; may be NULL; filled only when min_ssim != 0.  After the calls pngloss_hip_last_ssim and
 * pngloss_hip_multi_last_ssim return PNGLOSS_INVALID_ARGUMENT, like their distortion counterparts; the option "ssim" is left as the caller set it. */
int pngloss_hip_optimize_batch_target2(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                       const pngloss_hip_target2 *target, long bleed_divider, void *stream,
                                       pngloss_hip_result *results, pngloss_hip_target_report *reports, pngloss_hip_ssim *ssim);
int pngloss_hip_multi_optimize_batch_host_target2(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                                  const pngloss_hip_target2 *target, long bleed_divider, pngloss_hip_result *results,
                                                  pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                                  pngloss_hip_target_report *reports, pngloss_hip_ssim *ssim);

/* ---- A strength per image, found from a BYTE BUDGET (no reference equivalent).  The other half of a lossy compressor's contract: "make this
 * stream at most N bytes".  The originals stay on the device between the probes, the scanlines of every probe are emitted on the device, and the
 * device deflate -- the one that writes the streams of pngloss_hip_optimize_batch_host_zlib -- measures each probe's exact stream size without
 * writing the stream.
 *
 * A probe of an image at a strength is ACCEPTED when its status is 0 and its stream size is at most the image's max_bytes.  The stream size is
 * that of the complete zlib stream, 78 DA ... Adler-32: the number pngloss_hip_zstream.size reports for pngloss_hip_optimize_batch_host_zlib at
 * that strength.  The size is NOT guaranteed to be monotone in the strength, so the chosen strength is defined by this procedure, per image, with
 * M = max_strength:
 *     1. probe M; if it is refused, the chosen strength is M and reached = 0: the budget cannot be met below M, the image keeps the M result
 *     2. otherwise lo = -1 (virtual, refused), hi = M
 *     3. while hi - lo > 1: probe mid = (lo + hi) / 2, rounded down; accepted: hi = mid, otherwise lo = mid
 *     4. the chosen strength is hi and reached = 1
 * At most 1 + ceil(log2(M + 1)) probes.  Strength 0 is probed only when every probe above it passed: the lossless result, when it already fits.
 * A probe whose status is not 0 ends that image's search: the image keeps that probe's result and status, reached = 0.  An image without pixels
 * is chosen 0 with 0 probes (reached = 1, bytes = 0: it has no stream).
 * PNGLOSS_INVALID_ARGUMENT, before any image is touched: max_strength > 255; max_bytes NULL or max_bytes[i] == 0 for an image that has pixels; an
 * image with more than 1 GiB of scanlines ((4 * width + 1) * height, as for the _zlib form). */
typedef struct {
    const uint64_t *max_bytes;   /* n entries, indexed like images[]: the largest allowed zlib stream of image i */
    uint32_t max_strength;       /* M, 0..255: the search never goes above it */
    uint32_t reserved;           /* 0 */
} pngloss_hip_size_target;

typedef struct {
    uint32_t strength;           /* chosen */
    uint32_t probes;             /* probes of the rule above */
    uint32_t runs;               /* row-engine runs spent on this image */
    uint32_t reached;            /* 1: bytes <= max_bytes[i]; 0: not even M fits (or a probe failed) */
    uint64_t bytes;              /* measured size of the kept result's zlib stream; 0 for an image without pixels or a failed probe */
    int32_t  color_type;         /* of the kept result's scanlines: 0, 2, 4 or 6 */
    uint32_t reserved;           /* 0 */
    pngloss_hip_distortion distortion;   /* of the result that was kept, against the original */
} pngloss_hip_size_report;

/* The search on n device-resident images.  SYNCHRONOUS.  On return image i holds what pngloss_hip_optimize_batch at reports[i].strength writes,
 * byte for byte: pixels, d_row_filters and results[i] (results and reports may be NULL).  Every round the images still searching are grouped by
 * the strength they probe next; each group runs as one ordinary batch whose scanlines are emitted into the search arena, then ONE measuring
 * deflate takes the sizes of all images probed in the round and one copy of n small records brings them to the host (and one small copy per group
 * the colour types).  The plan, the engine choice
 * and the engines are those of pngloss_hip_optimize_batch.  No engine run is repeated: runs == probes.  The arena holds per image the original,
 * the best result so far with its row filters, and the scanlines of the current probe -- with `streams` also those of the best result so far --
 * (about 3, with streams 4, times width * height * 4 bytes per image; if it cannot be had the call returns PNGLOSS_OUT_OF_MEMORY_ERROR before any
 * image is touched).
 * streams: NULL, or n entries as for pngloss_hip_optimize_batch_host_zlib (data / capacity: room for pngloss_hip_zlib_bound(width, height) bytes;
 * flags are ignored).  One writing deflate over the kept results then fills them: streams[i] is byte for byte the stream _host_zlib gives for the
 * same image at reports[i].strength (with row filters when d_row_filters is given, without when it is NULL), and streams[i].size ==
 * reports[i].bytes.  This is also the way to a zlib stream of DEVICE-RESIDENT frames -- those of pngloss_hip_png_decode_batch_device, say --
 * without a host round trip of the pixels: a budget no stream can meet (1 byte) and max_strength = s is "strength s, stream wanted" -- one probe,
 * the image keeps the s result, reached = 0, and streams[i] is its stream.
 * After the call pngloss_hip_last_distortion, _last_ssim, _last_histogram and _last_engine_info return PNGLOSS_INVALID_ARGUMENT (no single batch
 * exists to index); the options "distortion" and "ssim" are left as the caller set them and play no part in the search. */
int pngloss_hip_optimize_batch_size(pngloss_hip_ctx *ctx, const pngloss_hip_image_desc *images, size_t n,
                                    const pngloss_hip_size_target *target, long bleed_divider, void *stream,
                                    pngloss_hip_result *results, pngloss_hip_zstream *streams, pngloss_hip_size_report *reports);

/* The same for host images over every context of `multi`, for the command line tool, as pngloss_hip_multi_optimize_batch_host_target: the images
 * are split over the contexts; each context uploads its images, finds their strengths with the search above (on copies: nothing is written
 * back), then runs the existing host-window path once per distinct chosen strength.  Outputs equal those of
 * pngloss_hip_multi_optimize_batch_host at reports[i].strength, image by image; this form spends one more run per image: runs == probes + 1.
 * results, scanlines, streams, reports may be NULL (independently).  After the call the _multi_last_* accessors return PNGLOSS_INVALID_ARGUMENT. */
int pngloss_hip_multi_optimize_batch_host_size(pngloss_hip_multi *multi, const pngloss_hip_host_image *images, size_t n,
                                               const pngloss_hip_size_target *target, long bleed_divider, pngloss_hip_result *results,
                                               pngloss_hip_scanlines *scanlines, pngloss_hip_zstream *streams,
                                               pngloss_hip_size_report *reports);

/* ---- PNG read side behind the inflate.  Replaces what libpng does for rwpng_read_image24_libpng
 * (/root/reference/src/rwpng.c:179-400) between "inflated IDAT bytes" and "RGBA8 rows": the inverse scanline filters (a recurrence over
 * x and y, run as a row wavefront on the device) and the transformations that reader registers -- palette / low bit depths / tRNS
 * expanded, 16-bit samples stripped to their high byte, gray to RGB, alpha 255 filled in (rwpng.c:239-258).  The caller parses the
 * chunks and inflates IDAT (zlib; pngloss_amd/cli/png_stream_reader.c does, on host threads) and passes
 *   scanlines     the inflated image data: height * (1 + rowbytes) bytes, filter type byte first in every row; for an Adam7-interlaced
 *                 image its seven passes one after another (each an image of its own, with its own rows and rowbytes; an empty pass has
 *                 no bytes at all)
 *   color_type, bit_depth, interlace   as in IHDR (interlace 0 = none, 1 = Adam7);  palette / palette_entries   the PLTE payload (RGB
 *                 triples);  trns / trns_bytes   the tRNS payload
 *   rgba          out: width * height * 4 bytes, exactly what rwpng_read_image24 returns in rgba_data (interlaced files are de-interlaced)
 * Zero-initialise these structs (and pngloss_hip_png_zsource below): members may be added where the layout has padding today, as
 * `interlace` was, and zero keeps the meaning they had before.
 * Returns PNGLOSS_SUCCESS, PNGLOSS_INVALID_ARGUMENT (not a PNG format, or an interlace method other than 0 and 1) or 25
 * (LIBPNG_FATAL_ERROR, rwpng.h:33: a filter type beyond 4, in any pass). */
typedef struct {
    const unsigned char *scanlines;
    uint32_t width, height;
    uint8_t color_type, bit_depth;
    uint8_t interlace;              /* 0 = none, 1 = Adam7 */
    const unsigned char *palette;
    uint32_t palette_entries;
    const unsigned char *trns;
    uint32_t trns_bytes;
    unsigned char *rgba;
} pngloss_hip_png_source;

int pngloss_hip_png_decode_batch_host(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n);
/* The same with a status per image (status: n ints or NULL): every image is decoded and downloaded whatever happens to the others, a damaged
 * one gets 25 in its slot (an internal failure PNGLOSS_HIP_ERROR) and the call returns the worst code -- the reference, too, fails only the
 * damaged file (/root/reference/src/pngloss.c:196-204).  Not while a batch is in flight on the context (PNGLOSS_INVALID_ARGUMENT).
 * A failure of the batch AS A WHOLE (bad argument, allocation, copy, launch, device fault: nothing was decoded) puts the call's return value
 * into EVERY status[i] (and NULL into every d_rgba[i] of the device forms): status[i] == 0 always means "image i is decoded". */
int pngloss_hip_png_decode_batch_host_status(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, int *status);

/* DEVICE-RESIDENT hand-over ("fuse with K0"): the same decode, but the RGBA8 images STAY in device memory -- in a frame
 * arena of the context, apart from the workspace the optimiser uses -- and d_rgba[i] receives their device pointers (width * height * 4 bytes,
 * 256-byte aligned), which go straight into pngloss_hip_image_desc.d_rgba of pngloss_hip_optimize_batch[_async] on the same context: the pixels
 * never travel back to the host between the reader and the optimiser (the classify / histogram kernels read what the expansion kernel
 * wrote).  src[i].rgba is not used (may be NULL).  The frames are valid until the next decode on this context, or its destruction; the
 * optimiser rewrites them in place.  Everything is enqueued on `stream` (a hipStream_t, NULL = the default stream); the call returns when the
 * statuses have arrived (the decode itself takes milliseconds).  status: n ints or NULL, as above.  Replaces the part of
 * /root/reference/src/rwpng.c:179-400 behind the inflate, like pngloss_hip_png_decode_batch_host. */
int pngloss_hip_png_decode_batch_device(pngloss_hip_ctx *ctx, const pngloss_hip_png_source *src, size_t n, void **d_rgba, int *status, void *stream);

/* The same from the COMPRESSED image data: the inflate, too, runs on the device -- one wave per file (pngloss_amd/csrc/pl_inflate_core.h: stored,
 * fixed and dynamic blocks, the 32 KB window in shared memory, Adler-32 checked), for the files of a window, whose streams are independent.
 * This replaces ALL of the reader behind the chunk walk (/root/reference/src/rwpng.c:179-400: libpng's png_read_image = zlib inflate + inverse
 * filters + transformations); what goes up is the file's compressed bytes, what comes out stays on the device.
 *   zstream   the concatenated payloads of the file's IDAT chunks (one zlib stream), zbytes of them; interlaced files (interlace = 1) too
 * A stream the device inflater does not take (damaged, preset dictionary, size mismatch ...) gets status 25 and the call returns 25: read that
 * file on the host (so does a stream shorter than 6 bytes or beyond 4 GiB -- that file only).  One wave decodes ~3 MB/s (profiles/r04_read_side.txt; zlib: ~250 MB/s per host thread): this pays only when a call brings well over
 * a thousand files; otherwise use the scanline form above, with zlib on host threads. */
typedef struct {
    const unsigned char *zstream;
    size_t zbytes;
    uint32_t width, height;
    uint8_t color_type, bit_depth;
    uint8_t interlace;              /* 0 = none, 1 = Adam7 */
    const unsigned char *palette;
    uint32_t palette_entries;
    const unsigned char *trns;
    uint32_t trns_bytes;
} pngloss_hip_png_zsource;

int pngloss_hip_png_decode_batch_device_z(pngloss_hip_ctx *ctx, const pngloss_hip_png_zsource *zsrc, size_t n, void **d_rgba, int *status, void *stream);

/* Page-locked host memory for what goes up to the device (the inflated scanlines handed to the decode calls, images handed to the host
 * batches): a copy from it is one DMA, a copy from pageable memory is staged by the runtime (33 ms against 1.3 ms for 64 MiB, bench.py
 * `transfers`).  NULL when the runtime has none to give; pngloss_hip_pinned_free(NULL) is a no-op. */
void *pngloss_hip_pinned_alloc(size_t bytes);
void pngloss_hip_pinned_free(void *p);

/* What the row engine did for image `index` of the last finished batch (diagnostics; bench.py reports it):
 *   info[0]  engine: 3 = segment-parallel (the image spread over the whole GPU: few large images, latency), 0 = one workgroup per image
 *            (batches), 4 = row statistics (every image of a batch at strength 0, where nothing is quantised and only the filter search of
 *            pngloss_image.c:201-287 is left: info[1] = rows).  Chosen per batch by pngloss_hip_optimize_batch_async from a cost model -- fitted on the reference kind of box, scaled by the device's CU count;
 *            PNGLOSS_HIP_CALIB=1 also calibrates it once per device and process on a small synthetic frame (~30 ms; off by default: the probe is sensitive to the clock governor) -- (wide images and small batches go to
 *            the segment-parallel engine, narrow images and large batches to the other; state sets of up to 1024 chain states, i.e.
 *            most strength / bleed pairs, rows up to 8192 pixels); PNGLOSS_HIP_ENGINE=seg|wg|lead|legacy|mix pins it (test hook).
 *   info[1]  row attempts (engine 3) / rows on the band-leader chains (engine 0)
 *   info[2]  validation restarts (engine 3) / pixels redone exactly (engine 0)
 *   info[3]  rows finished serially (engine 3) / rows on the round-1 chains by the adaptive choice (engine 0)
 *   info[4]  rows in which candidate none was ruled out by its cost bound (engine 3)
 *   info[5]  segments whose entry state was in no enumerated set (engine 3): walked step by step by the chain kernel (seeded state sets), or the
 *            places where a row was broken off and resumed in an epoch (exhaustive state sets: next to never from every state; a batch whose units or segments start from
 *            seeds -- round 6 -- breaks a row off where no seed reached its state and finishes it from every state)
 *   info[6]  launch groups the batch ran as (engine 3; see the option "launch_groups"), info[7] 1 when the call put a device-side wait for the engine on the
 *            caller's stream (the asynchronous entry's non-blocking variant), 0 when it waited on the host
 * No reference equivalent. */
int pngloss_hip_last_engine_info(pngloss_hip_ctx *ctx, size_t index, int32_t info[8]);

/* Options of a context (not while a batch is in flight).  Known: name "engine", value
 *   "auto"    (default) the row engine is chosen image by image from the cost model (see pngloss_hip_last_engine_info)
 *   "seg"     the segment-parallel engine for every image it takes (any strength / bleed; rows up to 2^20 pixels)
 *   "wg"      one workgroup per image (band-leader chains); "lead" / "legacy": its chain variants (diagnostics)
 *   "mix"     alternate the two engines over the images of a batch (diagnostics)
 *   "rows"    like "auto" (the row-statistics engine takes strength 0 under "auto" and "rows" alike; "seg" / "wg" run strength 0 the long way)
 * The environment variable PNGLOSS_HIP_ENGINE (the tests' hook) is read only while this option is at "auto" (once per call).
 * Name "launch_groups", value "auto" | "2" (default) | "3": how many launch sequences a large batch gets on the segment-parallel engine through the
 *   SYNCHRONOUS entry point pngloss_hip_optimize_batch.  "3" is 3-6 % faster at 32-64 frames of 1080p and is meant for a process that never gives
 *   pngloss_hip_optimize_batch_async a stream of its own: a third engine stream in the process slows every later engine run that waits on a caller's stream,
 *   so the library then runs the asynchronous entry in its blocking variant (it returns when the engine is done), and it never creates a third stream once
 *   any context of the process has used such a wait.
 * Name "distortion", value "on" | "off" (default): measure every batch from here on (pngloss_hip_last_distortion, above).  "off" launches exactly what
 *   the library launched before the option existed: no copy, no arena, no extra kernel.
 * Name "ssim", value "on" | "off" (default): measure the structural similarity of every batch from here on (pngloss_hip_last_ssim, above); independent of
 *   "distortion".  "off" launches exactly what the library launched before the option existed.
 * Name "measure", value "all" (default) | "visible": what the measuring kernels behind a batch ("distortion", "ssim") and the probes of the target searches
 *   (pngloss_hip_optimize_batch_target[2], pngloss_hip_multi_optimize_batch_host_target[2]) count: every pixel, or the visible ones on alpha-premultiplied
 *   channels ("Measuring over visible pixels", above).  No effect unless one of those measures; the byte-budget search always reports over all pixels.
 *   "all" launches exactly what the library launched before the option existed.
 * Name "indexed", value "on" | "off" (default): the calls that return zlib streams may answer with colour type 3 from here on (pngloss_hip_indexed.h,
 *   "Indexed-colour streams"; pngloss_hip_last_palette has the palette).  Like the options above it is read once, when a call begins, and travels with that batch.  "off"
 *   launches and writes exactly what the library did before the option existed.
 * Returns PNGLOSS_SUCCESS or PNGLOSS_INVALID_ARGUMENT (unknown name or value).
 * Results never depend on an option, on the engine, or on the environment: the remaining environment hooks (PNGLOSS_HIP_SEG_GROUPS, _SEG_UNIT, _ENUM_NT,
 * _NO_STREAM_WAIT, _SEGPROF, _DEBUG ...: timing and test pins) are read once, when a context is created, and none of them changes a byte; the debugging aid
 * that does ("candidate f wins every row") exists in builds made with -DPL_DEBUG_FORCE_FILTER=f only, and pngloss_hip_version() of such a build says so. */
int pngloss_hip_set_option(pngloss_hip_ctx *ctx, const char *name, const char *value);

/* Library / device identification string (static storage). */
const char *pngloss_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_H */

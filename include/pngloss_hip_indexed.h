/*
 * pngloss_hip_indexed.h -- the indexed-colour extension of the C ABI of libpngloss_hip.so (include/pngloss_hip.h, section 2): the record and the
 * accessors of the option "indexed".  Plain C; includes pngloss_hip.h.
 */
#ifndef PNGLOSS_HIP_INDEXED_H
#define PNGLOSS_HIP_INDEXED_H

#include "pngloss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Indexed-colour streams (no reference equivalent: the reference tool writes 8-bit gray, gray+alpha, RGB or RGBA, so every palette file that goes
 * in comes out as truecolour).  With the option "indexed" at "on" (pngloss_hip_set_option) the calls that return zlib streams --
 * pngloss_hip_optimize_batch_host_zlib, and pngloss_hip_multi_optimize_batch_host with streams != NULL -- also try PNG colour type 3 for every image
 * whose result has at most 256 colours, and keep whichever stream makes the smaller file.  Definitions, all exact:
 *   colours        the distinct 32-bit RGBA words of the final optimised RGBA8 image (what pngloss_hip_optimize_batch_host hands back)
 *   eligible       the image has pixels and 1 <= colours <= 256
 *   palette order  ascending by the pixel word read as a little-endian uint32: alpha most significant, then B, G, R -- so entries that are not opaque
 *                  come first; trns_entries is the number of entries with alpha != 255, and a tRNS chunk holds exactly the alphas of those first
 *                  entries (none when trns_entries is 0)
 *   indexed scanlines  colour type 3, bit depth 8: per row the filter type byte 0 ("none", what libpng uses for palette images) and `width` index
 *                  bytes.  Bit depths 1, 2 and 4 are written only where the option "index_depth" asks for them (pngloss_hip_index_depth.h).
 *   decision       T = size of the truecolour stream, I = size of the indexed one, both complete zlib streams as pngloss_hip_zstream.size counts them,
 *                  both written by the device deflate; overhead = 12 + 3 * entries + (trns_entries ? 12 + trns_entries : 0), the PLTE and tRNS
 *                  chunks.  Indexed is kept iff the image is eligible and I + overhead < T; a tie goes to truecolour.
 * Where indexed is kept, streams[i].color_type is 3 and streams[i].data / size / blocks are the indexed stream's (it always fits: it is smaller than
 * the truecolour one the buffer had room for).  The stream of every other image is byte for byte what the call writes with the option off; an image
 * that is not eligible costs one counting kernel (which leaves the image as soon as it has seen 257 colours) and nothing else.  Pixels, row filters,
 * results and the scanlines[] of the multi form (always the truecolour encoding) do not depend on the option; neither do the calls that return no
 * stream, and the device-resident searches (pngloss_hip_optimize_batch_target[2], pngloss_hip_optimize_batch_size) and their host forms ignore it: their
 * streams are truecolour.  The index workspace (per image 8 KiB of table and about width * height bytes of index rows) is allocated before anything is
 * enqueued: if it cannot be had the call returns PNGLOSS_OUT_OF_MEMORY_ERROR and nothing has run.
 *
 * The record of one image: what was decided, and from which numbers. */
typedef struct {
    uint32_t entries;          /* palette entries of the indexed stream; 0: this image was written as truecolour (then trns_entries, rgb and alpha are 0 too) */
    uint32_t trns_entries;     /* the first trns_entries entries have alpha != 255 */
    uint8_t  rgb[256][3];      /* the PLTE payload: entries * 3 bytes */
    uint8_t  alpha[256];       /* alpha of every entry; the tRNS payload is its first trns_entries bytes */
    uint64_t truecolor_bytes;  /* T; 0 for an image that got no stream (no pixels, status != 0, no buffer) */
    uint64_t indexed_bytes;    /* I; 0 when not eligible */
    uint32_t colors;           /* distinct colours; 257 = "more than 256"; 0 for an image that got no stream */
    uint32_t reserved;         /* 0 */
} pngloss_hip_palette;

/* Record of image `index` of the last finished call that returned zlib streams.  The rules of pngloss_hip_last_distortion: PNGLOSS_INVALID_ARGUMENT when
 * that batch ran with the option "indexed" off (or returned no streams), when the index is out of range or while a batch is pending; after a host
 * window that ran in chunks the index follows the chunks.  pngloss_hip_multi_last_palette: the record of images[index] of the last
 * pngloss_hip_multi_optimize_batch_host call, whichever context it went to. */
int pngloss_hip_last_palette(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_palette *out);
int pngloss_hip_multi_last_palette(pngloss_hip_multi *multi, size_t index, pngloss_hip_palette *out);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_INDEXED_H */

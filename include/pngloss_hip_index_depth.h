/*
 * pngloss_hip_index_depth.h -- the bit-depth extension of the indexed-colour write side of libpngloss_hip.so (include/pngloss_hip_indexed.h): the
 * option "index_depth", its record and the accessors.  Plain C; includes pngloss_hip_indexed.h.
 */
#ifndef PNGLOSS_HIP_INDEX_DEPTH_H
#define PNGLOSS_HIP_INDEX_DEPTH_H

#include "pngloss_hip_indexed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Palette streams at bit depths 1, 2 and 4 (no reference equivalent: the reference tool writes no palette files).  The option "index_depth"
 * (pngloss_hip_set_option, pngloss_hip_multi_set_option) is read only where the option "indexed" is on and the call returns zlib streams; the
 * searches ignore it as they ignore "indexed".  Definitions, all exact:
 *   min_depth(entries)  1 for 1..2 entries, 2 for 3..4, 4 for 5..16, 8 for 17..256 (0 for anything else: no palette)
 *   packed scanline at depth d in {1, 2, 4}: the filter type byte 0, then ceil(width * d / 8) bytes.  Pixel x lies in byte x * d / 8 at the shift
 *                       8 - d * (x % (8 / d) + 1): the leftmost pixel sits in the high bits, as PNG requires.  The unused low bits of a row's last
 *                       byte are 0.
 *   palette, palette order, tRNS, overhead: those of pngloss_hip_indexed.h, unchanged -- the depth changes the scanlines and nothing else.
 *   candidates          T: the truecolour stream; I8: the stream of the 8-bit index rows; Ip: the stream of the rows packed at min_depth, for an
 *                       eligible image with min_depth < 8.  Each is a complete zlib stream from the device deflate.
 * Values of the option:
 *   "8"     (default) what pngloss_hip_indexed.h states, bit for bit: T against I8, no packing kernel is launched.
 *   "auto"  the smallest of T, I8 + overhead and Ip + overhead is kept; a tie goes to the earlier one in that order.  Equivalently: the rule of
 *           "8" picks between T and I8, then the packed stream replaces the winner only where its file is strictly smaller.
 *   "min"   what other palette tools do: the candidates are T and the indexed stream at min_depth alone -- one deflate fewer; indexed is kept iff
 *           I + overhead < T.  For 17..256 colours this is "8".
 * Any other value is PNGLOSS_INVALID_ARGUMENT, and so is a call while a batch is pending.
 * Where a packed stream is kept, streams[i].color_type is 3 as for any indexed stream and the pngloss_hip_palette record is filled the same way;
 * pngloss_hip_zstream does not say the depth: this record does.  pngloss_hip_palette.indexed_bytes is the size of the indexed candidate that was
 * compared with T: under "auto" the smaller of I8 and Ip, under "min" the one at min_depth, under "8" I8 as before.  The workspace of the packed rows
 * (per image about width * height / 2 bytes) is allocated before anything is enqueued: if it cannot be had the call returns
 * PNGLOSS_OUT_OF_MEMORY_ERROR and nothing has run.  Packed rows carry filter type 0 only. */
typedef struct {
    uint32_t bit_depth;       /* of the stream that was kept: 0 truecolour, else 8, 4, 2 or 1 */
    uint32_t min_depth;       /* min_depth(colours) of an eligible image, else 0 */
    uint64_t indexed8_bytes;  /* I8; 0 where that candidate was not written */
    uint64_t packed_bytes;    /* Ip; 0 where there was no packed candidate */
} pngloss_hip_index_depth;

/* Record of image `index` of the last finished call that returned zlib streams with the option "indexed" on, whatever "index_depth" said (under "8"
 * bit_depth is 8 or 0).  The rules of pngloss_hip_last_palette, the multi form included.  (A host window that returns streams never runs in chunks, so an
 * index never has to follow any: after a window that did run in chunks there is no record.) */
int pngloss_hip_last_index_depth(pngloss_hip_ctx *ctx, size_t index, pngloss_hip_index_depth *out);
int pngloss_hip_multi_last_index_depth(pngloss_hip_multi *multi, size_t index, pngloss_hip_index_depth *out);

#ifdef __cplusplus
}
#endif
#endif /* PNGLOSS_HIP_INDEX_DEPTH_H */

/* png_stream_writer.h -- PNG container + zlib around scanlines that were filtered elsewhere (on the GPU). */
#ifndef PNGLOSS_AMD_PNG_STREAM_WRITER_H
#define PNGLOSS_AMD_PNG_STREAM_WRITER_H

#include "png_bridge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* chunk position flags as libpng records them while reading (png.h PNG_HAVE_IHDR / PNG_HAVE_PLTE / PNG_AFTER_IDAT) */
#define PNG_STREAM_HAVE_IHDR 0x01
#define PNG_STREAM_HAVE_PLTE 0x02
#define PNG_STREAM_AFTER_IDAT 0x08

typedef struct {
    uint32_t width, height;
    int color_type;                    /* 0 gray, 4 gray+alpha, 2 RGB, 6 RGBA, 3 indexed (`palette`); 8 bits per sample, and per index unless index_bits says less */
    const unsigned char *filter_ids;   /* [height] PNG filter type 0..4 of every scanline                       */
    const unsigned char *rows;         /* filtered scanline bytes, width*channels per row ...                   */
    size_t pitch;                      /* ... `pitch` bytes apart                                               */
    double gamma;                      /* written as gAMA when tag_gamma                                        */
    bool tag_gamma, tag_srgb;          /* what rwpng.c:508-516 of the reference derives from output_color       */
    const struct rwpng_chunk *chunks;  /* ancillary chunks to pass through (list order = write order)           */
    size_t maximum_file_size;          /* 0 = unlimited, else TOO_LARGE_FILE beyond it                          */
    const unsigned char *zdata;        /* optional: the finished zlib stream of the scanlines (GPU deflate); then    */
    size_t zsize;                      /* filter_ids/rows are not read and no zlib runs here                          */
    /* colour type 3 only (the library's option "indexed"): rows are `width` index bytes each.  PLTE follows the gAMA / sRGB tags and the chunks
     * passed through from in front of the input's PLTE, tRNS follows PLTE, both precede the first IDAT -- where libpng writes them */
    const unsigned char *palette;      /* palette_entries RGB triples, 1..256 of them: the PLTE payload               */
    unsigned palette_entries;
    const unsigned char *trns;         /* the alphas of the first trns_entries palette entries: the tRNS payload;      */
    unsigned trns_entries;             /* 0: no tRNS chunk is written                                                  */
    /* colour type 3 only (the library's option "index_depth"): the bit depth of the indices, IHDR byte 8.  Below 8 the rows are packed scanlines,
     * ceil(width * index_bits / 8) bytes each with the leftmost pixel in the high bits, and the palette has at most 1 << index_bits entries */
    unsigned index_bits;               /* 0 or 8: 8; else 1, 2 or 4 */
} png_stream_image;

pngloss_error png_stream_write(FILE *out, const png_stream_image *image, size_t *bytes_written, size_t *metadata_bytes);

/* How IDAT data is cut into chunks: zlib's output in libpng's 8192-byte slices; a finished stream from the GPU in chunks of 1 GiB (so: one) */
#define PNG_STREAM_ZLIB_IDAT_SLICE ((size_t)8192)
#define PNG_STREAM_GPU_IDAT_SLICE  ((size_t)1 << 30)

/* The size of the file png_stream_write writes for `image` when its zlib stream has stream_bytes bytes and goes out in IDAT chunks of at most
 * idat_slice bytes: signature, IHDR, the gAMA / sRGB tags, the pass-through chunks that will be copied, 12 bytes of framing per IDAT chunk, IEND.
 * Only width-independent fields of `image` are read (tags, chunks and, for colour type 3, the sizes of the palette and of tRNS): rows, filter ids
 * and zdata may be NULL. */
size_t png_stream_file_size(const png_stream_image *image, size_t stream_bytes, size_t idat_slice);

/* The other way round: the largest stream whose file is at most file_budget bytes; 0 when not even a 1-byte stream fits (the budget is smaller
 * than the container alone). */
size_t png_stream_largest_stream(const png_stream_image *image, size_t file_budget, size_t idat_slice);

#ifdef __cplusplus
}
#endif
#endif

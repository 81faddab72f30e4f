/* tests/c/stream_size.c -- test driver for the file-size helper of png_stream_writer.c: decode a PNG (png_bridge), take its scanlines unfiltered
 * in the colour type the writer side detects, write the file with png_stream_write twice -- zlib here, in 8192-byte IDAT slices; and from a
 * finished zlib stream, the way the GPU deflate's goes out -- and print what png_stream_file_size predicted next to what was written.
 * usage: stream_size in.png out_zlib.png out_stream.png strip
 * prints: predicted_zlib written_zlib predicted_stream written_stream stream_bytes largest(written) largest(written - 1) largest(container + 12) largest(container + 13) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "png_bridge.h"
#include "png_stream_writer.h"

/* the IDAT payload bytes of a PNG file on disk */
static size_t idat_bytes(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    unsigned char h[8];
    size_t total = 0;
    if (fread(h, 1, 8, f) != 8) { fclose(f); return 0; }
    while (fread(h, 1, 8, f) == 8) {
        const size_t n = ((size_t)h[0] << 24) | ((size_t)h[1] << 16) | ((size_t)h[2] << 8) | h[3];
        if (!memcmp(h + 4, "IDAT", 4)) total += n;
        if (fseek(f, (long)n + 4, SEEK_CUR)) break;
    }
    fclose(f);
    return total;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 1;
    const bool strip = atoi(argv[4]) != 0;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    png24_image img;
    memset(&img, 0, sizeof img);
    pngloss_error rc = rwpng_read_image24(in, &img, strip, false);
    fclose(in);
    if (rc) return (int)rc;
    const uint32_t W = img.width, H = img.height;
    bool gray = true, opaque = true;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const unsigned char *p = img.row_pointers[y] + 4 * x;
            gray = gray && p[0] == p[1] && p[1] == p[2];
            opaque = opaque && p[3] == 255;
        }
    const int ch = gray ? (opaque ? 1 : 2) : (opaque ? 3 : 4);
    const int ctype = gray ? (opaque ? 0 : 4) : (opaque ? 2 : 6);
    const size_t rb = (size_t)W * ch;
    unsigned char *raw = calloc(H ? H : 1, rb ? rb : 1), *ids = calloc(H ? H : 1, 1), *packed = calloc(H ? H : 1, rb + 1);
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const unsigned char *p = img.row_pointers[y] + 4 * x;
            unsigned char *d = raw + y * rb + (size_t)x * ch;
            if (ch == 1) d[0] = p[1]; else if (ch == 2) { d[0] = p[1]; d[1] = p[3]; } else if (ch == 3) { d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; } else memcpy(d, p, 4);
        }
        memcpy(packed + y * (rb + 1) + 1, raw + y * rb, rb);      /* filter type 0 in front of every row */
    }
    uLongf zcap = compressBound((uLong)((rb + 1) * H)), zsize = zcap;
    unsigned char *z = malloc(zcap);
    if (compress2(z, &zsize, packed, (uLong)((rb + 1) * H), 6) != Z_OK) return 3;
    png_stream_image si = { .width = W, .height = H, .color_type = ctype, .filter_ids = ids, .rows = raw, .pitch = rb, .gamma = img.gamma,
                            .tag_gamma = img.output_color != RWPNG_GAMA_ONLY && img.output_color != RWPNG_NONE,
                            .tag_srgb = img.output_color == RWPNG_SRGB, .chunks = img.chunks };
    FILE *o1 = fopen(argv[2], "wb");
    size_t n1 = 0, n2 = 0;
    rc = png_stream_write(o1, &si, &n1, NULL);
    fclose(o1);
    if (rc) return 40 + (int)rc;
    const size_t p1 = png_stream_file_size(&si, idat_bytes(argv[2]), PNG_STREAM_ZLIB_IDAT_SLICE);
    /* the prediction is made BEFORE the stream is attached, from the description alone, as the tool does */
    const size_t p2 = png_stream_file_size(&si, zsize, PNG_STREAM_GPU_IDAT_SLICE);
    const size_t container = png_stream_file_size(&si, 0, PNG_STREAM_GPU_IDAT_SLICE);
    si.zdata = z; si.zsize = zsize;
    FILE *o2 = fopen(argv[3], "wb");
    rc = png_stream_write(o2, &si, &n2, NULL);
    fclose(o2);
    if (rc) return 60 + (int)rc;
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", p1, n1, p2, n2, (size_t)zsize, png_stream_largest_stream(&si, n2, PNG_STREAM_GPU_IDAT_SLICE),
           png_stream_largest_stream(&si, n2 - 1, PNG_STREAM_GPU_IDAT_SLICE), png_stream_largest_stream(&si, container + 12, PNG_STREAM_GPU_IDAT_SLICE),
           png_stream_largest_stream(&si, container + 13, PNG_STREAM_GPU_IDAT_SLICE));
    return 0;
}

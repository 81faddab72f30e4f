/* tests/c/index_depth_write.c -- test driver for png_stream_writer.c with colour type 3 below 8 bits: a palette, an optional tRNS payload and packed
 * index rows go through png_stream_write, and the file that leaves is read back through the tool's own libpng bridge (png_bridge.c) to RGBA8.
 * usage: index_depth_write out.png out.rgba width height index_bits plte.bin trns.bin|- rows.bin stream.bin|-
 *   rows.bin: height rows of ceil(width * bits / 8) bytes (width bytes when index_bits is 0), which the writer deflates itself; with stream.bin
 *   the finished zlib stream of the scanlines goes out instead
 * prints: the writer's return code, bytes_written, what png_stream_file_size says, and the reader's return code */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "png_bridge.h"
#include "png_stream_writer.h"

static unsigned char *slurp(const char *path, size_t *n)
{
    *n = 0;
    if (strcmp(path, "-") == 0) return NULL;
    FILE *f = fopen(path, "rb");
    if (!f) exit(3);
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *p = malloc(len > 0 ? (size_t)len : 1);
    if (!p || (len > 0 && fread(p, (size_t)len, 1, f) != 1)) exit(3);
    fclose(f);
    *n = (size_t)len;
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    size_t plte_n, trns_n, rows_n, z_n;
    unsigned char *plte = slurp(argv[6], &plte_n), *trns = slurp(argv[7], &trns_n), *rows = slurp(argv[8], &rows_n), *z = slurp(argv[9], &z_n);
    const uint32_t width = (uint32_t)atol(argv[3]), height = (uint32_t)atol(argv[4]);
    const unsigned bits = (unsigned)atoi(argv[5]);
    unsigned char *ids = calloc(height ? height : 1, 1);
    if (!ids || !height || rows_n % height) return 3;
    /* (designated initialisers, as the tool's callers write them: a field that is not named is 0) */
    png_stream_image im = { .width = width, .height = height, .color_type = 3, .filter_ids = ids, .rows = rows, .pitch = rows_n / height,
                            .zdata = z, .zsize = z_n, .palette = plte, .palette_entries = (unsigned)(plte_n / 3), .trns = trns, .trns_entries = (unsigned)trns_n };
    if (bits) im.index_bits = bits;
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 3;
    size_t written = 0, meta = 0;
    const pngloss_error rc = png_stream_write(out, &im, &written, &meta);
    fclose(out);
    int read_rc = -1;
    if (rc == SUCCESS) {
        FILE *in = fopen(argv[1], "rb");
        if (!in) return 3;
        png24_image img;
        memset(&img, 0, sizeof img);
        read_rc = (int)rwpng_read_image24(in, &img, true, false);
        fclose(in);
        if (read_rc == SUCCESS && img.width == width && img.height == height) {
            FILE *raw = fopen(argv[2], "wb");
            if (!raw) return 3;
            for (uint32_t y = 0; y < height; y++) fwrite(img.row_pointers[y], 4, width, raw);
            fclose(raw);
        } else if (read_rc == SUCCESS) read_rc = -2;
        rwpng_free_image24(&img);
    }
    printf("%d %zu %zu %d\n", (int)rc, written, png_stream_file_size(&im, z ? z_n : 0, PNG_STREAM_GPU_IDAT_SLICE), read_rc);
    free(plte); free(trns); free(rows); free(z); free(ids);
    return 0;
}

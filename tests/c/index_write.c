/* tests/c/index_write.c -- test driver for png_stream_writer.c with colour type 3: a palette, an optional tRNS payload and a finished zlib stream
 * of index rows (made by the test with Python's zlib) go through png_stream_write; the test decodes the file with something else.
 * usage: index_write out.png width height plte.bin trns.bin|- stream.bin chunks max_file_size
 *   chunks: a string of b (a chunk recorded in front of the input's PLTE), m (between PLTE and IDAT) and a (behind IDAT); - for none
 * prints: the return code, bytes_written, metadata_bytes and what png_stream_file_size says for the same image */
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
    if (argc < 9) return 2;
    size_t plte_n, trns_n, z_n;
    unsigned char *plte = slurp(argv[4], &plte_n), *trns = slurp(argv[5], &trns_n), *z = slurp(argv[6], &z_n);
    static unsigned char before[] = "in front of PLTE", middle[] = "behind PLTE", after[] = "behind IDAT";
    struct rwpng_chunk cb = { NULL, before, sizeof before - 1, "prVt", PNG_STREAM_HAVE_IHDR };
    struct rwpng_chunk cm = { NULL, middle, sizeof middle - 1, "miDl", PNG_STREAM_HAVE_IHDR | PNG_STREAM_HAVE_PLTE };
    struct rwpng_chunk ca = { NULL, after, sizeof after - 1, "afTr", PNG_STREAM_HAVE_IHDR | PNG_STREAM_HAVE_PLTE | PNG_STREAM_AFTER_IDAT };
    struct rwpng_chunk *list = NULL, **tail = &list;
    for (const char *c = argv[7]; *c; c++) {
        struct rwpng_chunk *k = *c == 'b' ? &cb : *c == 'm' ? &cm : *c == 'a' ? &ca : NULL;
        if (k) { *tail = k; tail = &k->next; }
    }
    png_stream_image im;
    memset(&im, 0, sizeof im);
    im.width = (uint32_t)atol(argv[2]);
    im.height = (uint32_t)atol(argv[3]);
    im.color_type = 3;
    im.gamma = 0.45455;
    im.tag_gamma = true;
    im.tag_srgb = true;
    im.chunks = list;
    im.maximum_file_size = (size_t)atol(argv[8]);
    im.zdata = z;
    im.zsize = z_n;
    im.palette = plte;
    im.palette_entries = (unsigned)(plte_n / 3);
    im.trns = trns;
    im.trns_entries = (unsigned)trns_n;
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 3;
    size_t written = 0, meta = 0;
    const pngloss_error rc = png_stream_write(out, &im, &written, &meta);
    fclose(out);
    printf("%d %zu %zu %zu\n", (int)rc, written, meta, png_stream_file_size(&im, z_n, PNG_STREAM_GPU_IDAT_SLICE));
    free(plte); free(trns); free(z);
    return 0;
}

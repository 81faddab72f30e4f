/*
 * png_container_main.c -- TEST INFRASTRUCTURE: the command line tool's container reader (pngloss_amd/cli/png_stream_reader.c: signature, chunk walk with
 * CRC check, IHDR / PLTE / tRNS / gAMA / sRGB, inflate of the IDAT data with zlib) as a stand-alone program under -fsanitize=address,undefined
 * (tests/test_png_container_host.py compiles both files together and writes the hostile files).  Never shipped.
 *
 *   png_container_main file...
 * prints one line per file: "refuse", or
 *   "accept <width> <height> <colour type> <bit depth> <interlace> <palette entries> <palette, hex | -> <tRNS bytes> <tRNS, hex | -> <has tRNS> <has sRGB>
 *           <has gAMA> <gamma * 100000, rounded> <scanline bytes> <FNV-1a 64 of the scanlines, hex> <file size>"
 */
#include "../../pngloss_amd/cli/png_stream_reader.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static void hex(const unsigned char *p, size_t n)
{
    if (!n) { printf(" -"); return; }
    putchar(' ');
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        png_stream_source s;
        if (!png_stream_read(argv[a], &s)) {
            if (s.scanlines) { fprintf(stderr, "%s: refused, but scanlines are left behind\n", argv[a]); return 3; }
            puts("refuse");
            continue;
        }
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < s.scanline_bytes; i++) { h ^= s.scanlines[i]; h *= 0x100000001b3ull; }
        printf("accept %u %u %u %u %u %u", s.width, s.height, (unsigned)s.color_type, (unsigned)s.bit_depth, (unsigned)s.interlace, s.palette_entries);
        hex(s.palette, (size_t)s.palette_entries * 3);
        printf(" %u", s.trns_bytes);
        hex(s.trns, s.trns_bytes);
        printf(" %d %d %d %ld %zu %016llx %zu\n", (int)s.has_trns, (int)s.has_srgb, (int)s.has_gama, s.has_gama ? lround(s.gamma * 100000.0) : 0L, s.scanline_bytes,
               (unsigned long long)h, s.file_size);
        free(s.scanlines);
    }
    return 0;
}

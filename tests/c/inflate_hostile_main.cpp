/*
 * inflate_hostile_main.cpp -- TEST INFRASTRUCTURE: the device inflater's body (pngloss_amd/csrc/pl_inflate_core.h, the same source hipcc compiles
 * into pl_inflate.hip's kernel) as a stand-alone program under -fsanitize=address,undefined, stream by stream against zlib's inflate(Z_FINISH).
 * Never shipped, never loaded by the product.  (tests/test_inflate_hostile_host.py builds it twice: at the shipped PLI_IN and with -DPLI_IN=1024u.)
 *
 *   inflate_hostile_main <cases> <results>
 *     cases   : uint32 count, then per case uint32 zbytes, uint32 expect, zbytes bytes
 *     results : one text line per case: "<core status> <zlib accepts: 0 | 1> <verdict>", verdict being
 *                 ok       both accept and the bytes are equal, or both refuse
 *                 bytes    both accept, the bytes differ
 *                 refused  zlib accepts, the core refuses
 *                 accepted zlib refuses, the core accepts
 *
 * Every call gets fresh heap blocks of EXACTLY their size -- PliShared, the compressed bytes, the output --, filled with 0x5A (nothing may rely on zeroed
 * memory), so that a read behind the stream or a write behind the image is an AddressSanitizer report.  zlib accepts = inflate(Z_FINISH) into `expect`
 * bytes of room ends with Z_STREAM_END after exactly `expect` bytes.
 */
#include "../../pngloss_amd/csrc/pl_inflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <zlib.h>

static bool zlib_accepts(const unsigned char *z, unsigned zbytes, unsigned char *out, unsigned expect)
{
    z_stream s;
    std::memset(&s, 0, sizeof s);
    if (inflateInit(&s) != Z_OK) { std::fprintf(stderr, "inflateInit failed\n"); std::exit(2); }
    s.next_in = const_cast<unsigned char *>(z); s.avail_in = zbytes;
    s.next_out = out; s.avail_out = expect;
    const int r = inflate(&s, Z_FINISH);
    const bool ok = r == Z_STREAM_END && s.avail_out == 0;
    inflateEnd(&s);
    return ok;
}

static int core_status(const unsigned char *z, unsigned zbytes, unsigned char *out, unsigned expect)
{
    PliShared *S = static_cast<PliShared *>(std::malloc(sizeof(PliShared)));
    if (!S) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
    std::memset(S, 0x5A, sizeof *S);
    int32_t status = -1;
    const PliStream st{ z, zbytes, out, expect, &status };
    pli_inflate(st, *S);
    std::free(S);
    return status;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases results\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *res = std::fopen(argv[2], "w");
    if (!in || !res) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, in) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        uint32_t head[2];
        if (std::fread(head, 4, 2, in) != 2) return 2;
        const uint32_t zbytes = head[0], expect = head[1];
        unsigned char *z = static_cast<unsigned char *>(std::malloc(zbytes));
        unsigned char *got = static_cast<unsigned char *>(std::malloc(expect)), *want = static_cast<unsigned char *>(std::malloc(expect));
        if (!z || !got || !want) { std::fprintf(stderr, "out of memory\n"); return 2; }      /* (malloc(0) gives a block of no bytes here: any access to it is a report) */
        if (zbytes && std::fread(z, 1, zbytes, in) != zbytes) return 2;
        if (expect) { std::memset(got, 0x5A, expect); std::memset(want, 0xA5, expect); }
        const bool za = zlib_accepts(z, zbytes, want, expect);
        const int status = core_status(z, zbytes, got, expect);
        const char *verdict = "ok";
        if (za && status) verdict = "refused";
        else if (!za && !status) verdict = "accepted";
        else if (za && expect && std::memcmp(got, want, expect) != 0) verdict = "bytes";
        std::fprintf(res, "%d %d %s\n", status, za ? 1 : 0, verdict);
        std::free(z); std::free(got); std::free(want);
    }
    std::fclose(in);
    return std::fclose(res) == 0 ? 0 : 2;
}

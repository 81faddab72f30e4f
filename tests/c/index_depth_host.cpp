/* tests/c/index_depth_host.cpp -- test infrastructure: what pngloss_amd/csrc/pl_index_core.h and pl_layout.h add for the option "index_depth", run on
 * the CPU under the sanitizers: the body of pl_index_pack the way the kernel runs it, the rule that names the stream to keep, and the layout of
 * the packed rows.
 * usage: index_depth_host pack cases.bin out.bin
 *            cases.bin: u32 n; per case u32 depth, width, height; height * width index bytes
 *            out.bin:   per case u32 pitch8, pitch; height * pitch bytes: the packed rows, 0xEE where nothing was written
 *            The 8-bit rows are laid out as pl_index_layout lays them out, in an allocation that ends with the last row's pitch, and every byte
 *            behind `width` is 0xFF.  The packed rows are held against a restatement that places one pixel at a time; a difference is exit code 10.
 *        index_depth_host rule          stdin: lines "mode colors T I8 Ip trns"; stdout: "keep_depth indexed_candidate wants8 wantsp" each
 *        index_depth_host min_depth     stdout: min_depth(0) .. min_depth(257)
 *        index_depth_host layout w h [w h ...]   stdout: "index_total jobs total", then per image "ids rows pitch rows8 pitch8" */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pngloss_amd/csrc/pl_layout.h"

namespace {

/* what pl_index.h states about a job record (the header itself needs the HIP runtime) */
constexpr size_t kIndexJobBytes = 72, kPackJobBytes = 48;

bool read_u32(FILE *f, uint32_t *v, size_t n) { return fread(v, sizeof(uint32_t), n, f) == n; }

/* the definition, one pixel at a time: pixel x in byte x * d / 8 at the shift 8 - d * (x % (8 / d) + 1) */
std::vector<uint8_t> restate_row(const uint8_t *idx, uint32_t W, uint32_t d)
{
    std::vector<uint8_t> row(((size_t)W * d + 7) / 8, 0);
    for (uint32_t x = 0; x < W; x++) row[(size_t)x * d / 8] |= (uint8_t)(idx[x] << (8 - d * (x % (8 / d) + 1)));
    return row;
}

int pack(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!read_u32(in, &ncases, 1)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t head[3];
        if (!read_u32(in, head, 3)) return 3;
        const uint32_t d = head[0], W = head[1], H = head[2];
        if (!(d == 1 || d == 2 || d == 4) || !W || !H) return 3;
        std::vector<uint8_t> idx((size_t)W * H);
        if (fread(idx.data(), 1, idx.size(), in) != idx.size()) return 3;
        const PlIndexLayout ilay = pl_index_layout({ W }, { H }, kIndexJobBytes, sizeof(PliRecord));
        const PlPackLayout play = pl_index_pack_layout({ W }, { H }, ilay.total, kPackJobBytes);
        const uint32_t pitch8 = ilay.im[0].pitch, pitch = play.im[0].pitch;
        if (pitch8 % 16 || pitch8 < W || pitch % 16 || pitch < 4 * pli_packed_dwords(W, d)) return 4;
        /* the 8-bit rows: exactly height * pitch8 bytes, so that a load behind the last row's pitch is a sanitizer report */
        uint8_t *rows8 = static_cast<uint8_t *>(aligned_alloc(16, (size_t)pitch8 * H));
        if (!rows8) return 5;
        memset(rows8, 0xFF, (size_t)pitch8 * H);
        for (uint32_t y = 0; y < H; y++) memcpy(rows8 + (size_t)y * pitch8, idx.data() + (size_t)y * W, W);
        std::vector<uint8_t> rows((size_t)pitch * H, 0xEE);
        const uint32_t dwords = pli_packed_dwords(W, d);
        /* pl_index_pack: the lanes one after the other */
        for (uint32_t y = 0; y < H; y++) {
            for (uint32_t q = 0; q < dwords; q++) {
                const uint32_t v = pli_pack_lane_at(d, rows8 + (size_t)y * pitch8, W, q);
                uint8_t *dst = rows.data() + (size_t)y * pitch + 4 * (size_t)q;
                for (int b = 0; b < 4; b++) dst[b] = (uint8_t)(v >> (8 * b));          /* memory order: the first byte is the low one */
            }
        }
        free(rows8);
        for (uint32_t y = 0; y < H; y++) {
            const std::vector<uint8_t> want = restate_row(idx.data() + (size_t)y * W, W, d);
            const uint8_t *got = rows.data() + (size_t)y * pitch;
            if (want.size() != pli_packed_rowbytes(W, d)) return 10;
            for (uint32_t b = 0; b < pitch; b++) {
                const uint8_t w = b < want.size() ? want[b] : b < 4 * dwords ? 0 : 0xEE;
                if (got[b] != w) { fprintf(stderr, "depth %u width %u row %u byte %u: %02x, restated %02x\n", d, W, y, b, got[b], w); return 10; }
            }
        }
        const uint32_t headout[2] = { pitch8, pitch };
        fwrite(headout, sizeof headout, 1, out);
        fwrite(rows.data(), 1, rows.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 5;
}

int rule()
{
    unsigned mode, colors, trns;
    unsigned long long T, I8, Ip;
    while (scanf("%u %u %llu %llu %llu %u", &mode, &colors, &T, &I8, &Ip, &trns) == 6)
        printf("%u %llu %d %d\n", pli_keep_depth(mode, colors, I8, Ip, T, trns), (unsigned long long)pli_indexed_candidate(mode, colors, I8, Ip),
               (int)pli_wants_indexed8(mode, colors), (int)pli_wants_packed(mode, colors));
    return 0;
}

int layout(int n, char **dims)
{
    std::vector<uint32_t> width, height;
    for (int k = 0; k + 1 < n; k += 2) { width.push_back((uint32_t)strtoul(dims[k], nullptr, 10)); height.push_back((uint32_t)strtoul(dims[k + 1], nullptr, 10)); }
    const PlIndexLayout ilay = pl_index_layout(width, height, kIndexJobBytes, sizeof(PliRecord));
    const PlIndexLayout again = pl_index_layout(width, height, kIndexJobBytes, sizeof(PliRecord));
    const PlPackLayout play = pl_index_pack_layout(width, height, ilay.total, kPackJobBytes);
    if (again.total != ilay.total) return 4;
    printf("%zu %zu %zu\n", ilay.total, play.jobs, play.total);
    for (size_t i = 0; i < width.size(); i++)
        printf("%zu %zu %u %zu %u\n", play.im[i].ids, play.im[i].rows, play.im[i].pitch, ilay.im[i].rows, ilay.im[i].pitch);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "pack")) return pack(argv[2], argv[3]);
    if (argc >= 2 && !strcmp(argv[1], "rule")) return rule();
    if (argc >= 2 && !strcmp(argv[1], "min_depth")) {
        for (uint32_t e = 0; e <= 257; e++) printf("%u\n", pli_min_depth(e));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "layout")) return layout(argc - 2, argv + 2);
    return 2;
}

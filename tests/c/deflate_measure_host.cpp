/*
 * deflate_measure_host.cpp -- TEST INFRASTRUCTURE: the measure-only mode of both block encoders (pngloss_amd/csrc/pl_deflate_core.h,
 * pl_deflate_coop.h) and the per-image fold of dfl_sizes on the CPU.  Built with -fsanitize=address,undefined and run by
 * tests/test_deflate_measure_host.py.  In measure mode the encoders get NO output buffer (NULL): a single byte written would be a report.
 * Never shipped.
 *
 *   deflate_measure_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   D IN OUT BLOCK_BYTES TEAM...  the bytes of file IN as one image, in blocks of BLOCK_BYTES; per TEAM (0: the one-thread encoder, N >= 1:
 *                                 dfl_encode_block_coop with N host threads) every block is encoded in both modes; the writing mode's zlib
 *                                 stream goes to file OUT.TEAM (empty input: no stream, as in the product).
 *                                 -> per TEAM, separated by "|": nblocks record.bytes record.adler kinds_0 kinds_1 kinds_2, then per block
 *                                    w.bytes w.kind w.tokens w.adler_a w.adler_b m.bytes m.kind m.tokens m.adler_a m.adler_b
 *                                 The record is folded from the MEASURING mode's results by the thread loop of dfl_sizes, with 64 lanes.
 */
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>

#define DFL_COOP_MAX_BLOCK (1u << 22)          /* the tests also use blocks other than the product's 256 KiB */
#include "../../pngloss_amd/csrc/pl_deflate_coop.h"

static void barrier_wait(void *b) { pthread_barrier_wait(static_cast<pthread_barrier_t *>(b)); }

static dfl_block_result encode(int team, uint32_t mode, const uint8_t *in, const uint32_t *match, const uint32_t *near, const dfl_block_desc *d,
                               const dfl_params *prm, uint32_t *tok, uint32_t *choice, uint8_t *out)
{
    if (team == 0) {
        static dfl_work work;
        dfl_block_result r = dfl_encode_block_mode(in, match, near, d, prm, tok, choice, out, &work, mode);
        dfl_adler_partial(in, d->begin, d->end, 0, 1, &r.adler_a, &r.adler_b);
        return r;
    }
    static dfl_coop shared;                      /* the team's "LDS" */
    dfl_block_result res{};
    if (team == 1) {
        dfl_team t = { 0, 1, nullptr, nullptr };
        return dfl_encode_block_coop_mode(&t, in, match, near, d, prm, tok, choice, out, &shared, mode);
    }
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, (unsigned)team);
    std::vector<std::thread> th;
    for (int i = 0; i < team; i++)
        th.emplace_back([&, i] {
            dfl_team t = { (uint32_t)i, (uint32_t)team, barrier_wait, &bar };
            const dfl_block_result r = dfl_encode_block_coop_mode(&t, in, match, near, d, prm, tok, choice, out, &shared, mode);
            if (i == 0) res = r;
        });
    for (auto &x : th) x.join();
    pthread_barrier_destroy(&bar);
    return res;
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream cmdline(line);
        std::string cmd, in_path, out_path;
        uint32_t block_bytes = 0;
        if (!(cmdline >> cmd)) continue;
        if (cmd != "D" || !(cmdline >> in_path >> out_path >> block_bytes) || !block_bytes || block_bytes > DFL_COOP_MAX_BLOCK) return 2;
        std::vector<int> teams;
        for (int v; cmdline >> v;) { if (v < 0 || v > 256) return 2; teams.push_back(v); }
        std::vector<uint8_t> data;
        {
            FILE *g = std::fopen(in_path.c_str(), "rb");
            if (!g) return 2;
            uint8_t tmp[65536];
            size_t got;
            while ((got = std::fread(tmp, 1, sizeof tmp, g)) > 0) data.insert(data.end(), tmp, tmp + got);
            std::fclose(g);
        }
        const uint32_t n = (uint32_t)data.size();
        data.resize((size_t)n + 512, 0);           /* slack: the key / compare loads may run past the end, as on the device */
        const uint8_t *in = data.data();
        /* the match search of the product, serially (tests/c/deflate_host.cpp has the same loop) */
        const dfl_params prm = { DFL_DEFAULT_MAX_CHAIN, DFL_KEY_BYTES, block_bytes };
        static const uint32_t levels[] = DFL_DEFAULT_LEVELS;
        std::vector<uint32_t> key(n), skey(n), sorted(n), rank(n), gstart(n), match(n, 0u), near(n), tok(block_bytes), choice((size_t)n + 1);
        for (size_t lv = 0; lv < sizeof levels / sizeof levels[0]; lv++) {
            for (uint32_t p = 0; p < n; p++) key[p] = dfl_sort_key(in, p, n, levels[lv]);
            std::iota(sorted.begin(), sorted.end(), 0u);
            std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
            for (uint32_t i = 0; i < n; i++) {
                rank[sorted[i]] = i;
                skey[i] = key[sorted[i]];
                gstart[i] = (i && skey[i] == skey[i - 1]) ? gstart[i - 1] : i;
            }
            for (uint32_t p = 0; p < n; p++)
                match[p] = dfl_search_level(in, 0, n, p, sorted.data(), rank[p], gstart[rank[p]], dfl_level_chain(prm.max_chain, levels[lv]), levels[lv], lv ? levels[lv - 1] : 0u, match[p]);
        }
        for (uint32_t p = 0; p < n; p++) near[p] = dfl_near_match(in, 0, n, p);

        std::vector<dfl_block_desc> desc;
        for (uint32_t b0 = 0; b0 < n; b0 += block_bytes) {
            const uint32_t bl = std::min(block_bytes, n - b0);
            desc.push_back(dfl_block_desc{ b0, b0 + bl, 0, n, 0, 0, dfl_block_bound(bl), b0 + bl == n ? 1u : 0u });
        }
        bool first_team = true;
        for (const int team : teams) {
        std::vector<dfl_block_result> wres, mres;
        std::vector<uint8_t> stream, buf(dfl_block_bound(block_bytes) + 16);
        for (const dfl_block_desc &d : desc) {
            std::memset(buf.data(), 0, buf.size());
            wres.push_back(encode(team, DFL_MODE_WRITE, in, match.data(), near.data(), &d, &prm, tok.data(), choice.data(), buf.data()));
            if (wres.back().bytes > buf.size()) return 3;
            stream.insert(stream.end(), buf.begin(), buf.begin() + wres.back().bytes);
            std::fill(tok.begin(), tok.end(), 0u);
            std::fill(choice.begin(), choice.end(), 0u);
            mres.push_back(encode(team, DFL_MODE_MEASURE, in, match.data(), near.data(), &d, &prm, tok.data(), choice.data(), nullptr));
        }
        /* the fold of dfl_sizes: 64 lanes add sizes and kinds up, the Adler-32 composes in stream order */
        dfl_size_record rec{};
        const uint32_t nb = (uint32_t)desc.size();
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint64_t bytes;
            uint32_t kinds[3];
            dfl_size_partial(mres.data(), 0, nb, lane, 64, &bytes, kinds);
            rec.bytes += bytes;
            for (int k = 0; k < 3; k++) rec.kinds[k] += kinds[k];
        }
        rec.bytes = nb ? DFL_ZLIB_HEAD_BYTES + rec.bytes + DFL_ZLIB_TAIL_BYTES : 0;
        rec.adler = dfl_size_adler(mres.data(), desc.data(), 0, nb);
        {
            FILE *g = std::fopen((out_path + "." + std::to_string(team)).c_str(), "wb");
            if (!g) return 2;
            if (nb) {
                uint32_t adler = 1;
                for (uint32_t b = 0; b < nb; b++) adler = dfl_adler_fold(adler, wres[b].adler_a, wres[b].adler_b, desc[b].end - desc[b].begin);
                const uint8_t head[2] = { 0x78, 0xda }, tail[4] = { (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler };
                std::fwrite(head, 1, 2, g);
                std::fwrite(stream.data(), 1, stream.size(), g);
                std::fwrite(tail, 1, 4, g);
            }
            std::fclose(g);
        }
        std::printf("%s%u %" PRIu64 " %u %u %u %u", first_team ? "" : " | ", nb, rec.bytes, rec.adler, rec.kinds[0], rec.kinds[1], rec.kinds[2]);
        for (uint32_t b = 0; b < nb; b++)
            std::printf(" %u %u %u %u %" PRIu64 " %u %u %u %u %" PRIu64, wres[b].bytes, wres[b].kind, wres[b].tokens, wres[b].adler_a, wres[b].adler_b,
                        mres[b].bytes, mres[b].kind, mres[b].tokens, mres[b].adler_a, mres[b].adler_b);
        first_team = false;
        }
        std::printf("\n");
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

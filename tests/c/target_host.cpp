/*
 * target_host.cpp -- TEST INFRASTRUCTURE: the decisions of pngloss_hip_optimize_batch_target (pngloss_amd/csrc/pl_target.h) and the thread loop of its
 * copy kernel (pl_move_core.h) on the CPU.  Built with -fsanitize=address,undefined and run by tests/test_target_host.py, which compares every line
 * with a restatement of the rule in Python.  Never shipped.
 *
 *   target_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   S M TABLE         search below M; TABLE is a string of M + 1 characters '0' / '1': is a probe at strength s accepted.
 *                     -> chosen probes bound probe_1 probe_2 ...
 *   F M TABLE K       the same, but probe number K (1-based) comes back with a status other than 0 -> chosen probes failed(0/1) probe_1 ...
 *   A PSNRBITS MAXABS M STATUS BPP PIXELS CHANGED SQ0 SQ1 SQ2 SQ3 MX0 MX1 MX2 MX3   (PSNRBITS: the double's bits, hexadecimal) -> 0 / 1
 *   C PSNRBITS MAXABS M                -> the code pl_target_check gives
 *   G NEXT_0 NEXT_1 ...                a round of searches that probe NEXT_i next (-1: finished) -> strength:i,i,... per group
 *   L HOST W_0 H_0 W_1 H_1 ...         the search arena -> total, then per image orig best best_filters img filters
 *   M BYTES SRC_OFFSET DST_OFFSET NTHREADS   BYTES pseudo-random bytes copied by plm_thread between heap blocks that start that many bytes behind a
 *                     16-byte boundary and end with their last byte -> 1 if the copy equals the source
 */
#include "../../pngloss_amd/csrc/pl_target.h"
#include "../../pngloss_amd/csrc/pl_move_core.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

static double from_bits(const std::string &hex)
{
    const uint64_t b = std::strtoull(hex.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "S" || cmd == "F") {
            uint32_t M = 0, fail_at = 0;
            std::string table;
            in >> M >> table;
            if (cmd == "F") in >> fail_at;
            if (M > 255 || table.size() != (size_t)M + 1) return 2;
            PlTargetSearch s = pl_target_begin(M);
            std::string seq;
            while (!s.done) {
                if (s.next > M) return 3;                      /* the search never goes above M */
                seq += " " + std::to_string(s.next);
                if (fail_at && s.probes + 1 == fail_at) pl_target_fail(s);
                else pl_target_step(s, table[s.next] == '1');
            }
            if (cmd == "S") std::printf("%u %u %u%s\n", s.chosen, s.probes, pl_target_probe_bound(M), seq.c_str());
            else std::printf("%u %u %d%s\n", s.chosen, s.probes, s.failed ? 1 : 0, seq.c_str());
        } else if (cmd == "A" || cmd == "C") {
            std::string bits;
            pngloss_hip_target t{};
            in >> bits >> t.max_abs_error >> t.max_strength;
            t.min_psnr_db = from_bits(bits);
            if (cmd == "C") { std::printf("%d\n", pl_target_check(&t)); continue; }
            int32_t status = 0;
            uint32_t bpp = 0;
            pngloss_hip_distortion r{};
            in >> status >> bpp >> r.pixels >> r.changed_pixels;
            for (int c = 0; c < 4; c++) in >> r.sq_err[c];
            for (int c = 0; c < 4; c++) in >> r.max_abs[c];
            if (!in) return 2;
            std::printf("%d\n", pl_target_accept(t, r, status, bpp) ? 1 : 0);
        } else if (cmd == "G") {
            std::vector<PlTargetSearch> s;
            for (long v; in >> v;) {
                PlTargetSearch one = pl_target_begin(v < 0 ? 0 : (uint32_t)v);
                one.done = v < 0;
                s.push_back(one);
            }
            std::string out;
            for (const auto &g : pl_target_groups(s)) {
                out += (out.empty() ? "" : " ") + std::to_string(g.first) + ":";
                for (size_t k = 0; k < g.second.size(); k++) out += (k ? "," : "") + std::to_string(g.second[k]);
            }
            std::printf("%s\n", out.c_str());
        } else if (cmd == "L") {
            int host = 0;
            in >> host;
            std::vector<uint32_t> w, h;
            for (uint32_t a, b; in >> a >> b;) { w.push_back(a); h.push_back(b); }
            const PlTargetLayout lay = pl_target_layout(w, h, host != 0, 24, 32, 64);
            std::printf("%zu %zu %zu %zu", lay.total, lay.moves, lay.jobs, lay.records);
            for (const PlTargetImage &m : lay.image) std::printf(" %zu %zu %zu %zu %zu", m.orig, m.best, m.best_filters, m.img, m.filters);
            std::printf("\n");
        } else if (cmd == "M") {
            size_t bytes = 0, so = 0, dof = 0, nt = 0;
            in >> bytes >> so >> dof >> nt;
            if (!in || so >= 16 || dof >= 16 || !nt) return 2;
            void *bs = nullptr, *bd = nullptr;
            /* (the blocks end with the last byte, so a load or store past a range is a report) */
            if (posix_memalign(&bs, 16, bytes + so ? bytes + so : 1) || posix_memalign(&bd, 16, bytes + dof ? bytes + dof : 1)) return 2;
            uint8_t *src = static_cast<uint8_t *>(bs) + so, *dst = static_cast<uint8_t *>(bd) + dof;
            uint32_t lcg = (uint32_t)(bytes * 2654435761u + so * 17 + dof);
            for (size_t i = 0; i < bytes; i++) { lcg = lcg * 1664525u + 1013904223u; src[i] = (uint8_t)(lcg >> 24); dst[i] = (uint8_t)~src[i]; }
            for (size_t tid = 0; tid < nt; tid++) plm_thread(src, dst, bytes, tid, nt);
            std::printf("%d\n", std::memcmp(src, dst, bytes) == 0 ? 1 : 0);
            std::free(bs);
            std::free(bd);
        } else return 2;
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

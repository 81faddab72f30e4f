/*
 * colors_host.cpp -- TEST INFRASTRUCTURE: the decisions of pngloss_hip_quantize_batch_target (pngloss_amd/csrc/pl_colors.h) on the CPU.  Built with
 * -fsanitize=address,undefined and run by tests/test_quant_target_host.py, which compares every line with a restatement of the rule in Python.
 * Never shipped.
 *
 *   colors_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   S M TABLE         search up to M; TABLE is a string of M + 1 characters '0' / '1': is a probe at N colours accepted.
 *                     -> chosen reached probes bound accepted_mask probe_1 probe_2 ...   (the probes as the report's `probed` lists them)
 *   E M PIXELS COLORS_IN   the probes an image takes without device work (pl_colors_settle) from the start of its search
 *                     -> stepped done chosen reached next
 *   A PSNRBITS MAXABS PIXELS CHANGED SQ0 SQ1 SQ2 SQ3 MX0 MX1 MX2 MX3   (PSNRBITS: the double's bits, hexadecimal) -> 0 / 1
 *   C PSNRBITS MAXABS RESERVED         -> the code pl_colors_target_check gives ("C null": for no target at all)
 *   G NEXT_0 NEXT_1 ...                a round of searches that probe NEXT_i next (-1: finished) -> image:N per job
 */
#include "../../pngloss_amd/csrc/pl_colors.h"

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
        if (cmd == "S") {
            uint32_t M = 0;
            std::string table;
            in >> M >> table;
            if (M < 2 || M > 256 || table.size() != (size_t)M + 1) return 2;
            PlColorsSearch s = pl_colors_begin(M);
            while (!s.done) {
                if (s.next > M || s.next < 2) return 3;       /* the search never leaves 2 .. M */
                pl_colors_step(s, table[s.next] == '1');
            }
            if (s.probes > PLC_MAX_PROBES) return 3;
            std::printf("%u %d %u %u %u", s.chosen, s.reached ? 1 : 0, s.probes, pl_colors_probe_bound(M), s.accepted_mask);
            for (uint32_t k = 0; k < PLC_MAX_PROBES; k++) {
                if (k < s.probes) std::printf(" %u", s.probed[k]);
                else if (s.probed[k]) return 3;                /* the rest is 0 */
            }
            std::printf("\n");
        } else if (cmd == "E") {
            uint32_t M = 0, colors_in = 0;
            uint64_t pixels = 0;
            in >> M >> pixels >> colors_in;
            if (!in) return 2;
            PlColorsSearch s = pl_colors_begin(M);
            const uint32_t stepped = pl_colors_settle(s, pixels, colors_in);
            std::printf("%u %d %u %d %u\n", stepped, s.done ? 1 : 0, s.chosen, s.reached ? 1 : 0, s.next);
        } else if (cmd == "A" || cmd == "C") {
            std::string bits;
            pngloss_hip_quant_target t{};
            in >> bits;
            if (cmd == "C" && bits == "null") { std::printf("%d\n", pl_colors_target_check(nullptr)); continue; }
            in >> t.max_abs_error;
            t.min_psnr_db = from_bits(bits);
            if (cmd == "C") {
                in >> t.reserved;
                if (!in) return 2;
                std::printf("%d\n", pl_colors_target_check(&t));
                continue;
            }
            PlDistortRecord r{};
            in >> r.pixels >> r.changed_pixels;
            for (int c = 0; c < 4; c++) in >> r.sq_err[c];
            for (int c = 0; c < 4; c++) in >> r.max_abs[c];
            if (!in) return 2;
            std::printf("%d\n", pl_colors_accept(t, r) ? 1 : 0);
        } else if (cmd == "G") {
            std::vector<PlColorsSearch> s;
            for (long v; in >> v;) {
                PlColorsSearch one = pl_colors_begin(v < 0 ? 2 : (uint32_t)v);
                one.done = v < 0;
                s.push_back(one);
            }
            std::string out;
            for (const auto &job : pl_colors_round(s)) out += (out.empty() ? "" : " ") + std::to_string(job.first) + ":" + std::to_string(job.second);
            std::printf("%s\n", out.c_str());
        } else return 2;
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

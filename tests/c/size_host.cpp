/*
 * size_host.cpp -- TEST INFRASTRUCTURE: the decisions of pngloss_hip_optimize_batch_size (pngloss_amd/csrc/pl_size.h) and the search arena with
 * its scanline regions (pl_target.h) on the CPU.  Built with -fsanitize=address,undefined and run by tests/test_size_host.py, which compares
 * every line with a restatement of the rule in Python (tests/util_size.py).  Never shipped.
 *
 *   size_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   S M TABLE         search below M; TABLE is a string of M + 1 characters '0' / '1': is a probe at strength s accepted.
 *                     -> chosen reached probes bound probe_1 probe_2 ...
 *   F M TABLE K       the same, but probe number K (1-based) comes back with a status other than 0 -> chosen reached probes failed(0/1) probe_1 ...
 *   E M               an image without pixels -> chosen reached probes done(0/1)
 *   A STATUS BYTES MAX                 -> 0 / 1: pl_size_accept
 *   C M NULLBUDGETS W_0 H_0 B_0 W_1 H_1 B_1 ...   -> the code pl_size_check gives (NULLBUDGETS 1: max_bytes == NULL)
 *   G NEXT_0 NEXT_1 ...                a round of searches that probe NEXT_i next (-1: finished) -> strength:i,i,... per group
 *   L HOST SCAN W_0 H_0 W_1 H_1 ...    the search arena, scanline regions SCAN = 0 / 1 / 2 -> total moves jobs records flags, then per image
 *                                      orig best best_filters img filters rows ids best_rows best_ids pitch
 *   R                                  -> sizeof(PlSizeRecord) and the offsets of bytes, adler, kinds
 */
#include "../../pngloss_amd/csrc/pl_size.h"
#include "../../pngloss_amd/csrc/pl_target.h"
#include "../../pngloss_amd/csrc/pl_layout.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

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
            PlSizeSearch s = pl_size_begin(M, true);
            std::string seq;
            while (!s.done) {
                if (s.next > M) return 3;                      /* the search never goes above M */
                seq += " " + std::to_string(s.next);
                if (fail_at && s.probes + 1 == fail_at) pl_size_fail(s);
                else pl_size_step(s, table[s.next] == '1');
            }
            if (cmd == "S") std::printf("%u %u %u %u%s\n", s.chosen, s.reached, s.probes, pl_size_probe_bound(M), seq.c_str());
            else std::printf("%u %u %u %d%s\n", s.chosen, s.reached, s.probes, s.failed ? 1 : 0, seq.c_str());
        } else if (cmd == "E") {
            uint32_t M = 0;
            in >> M;
            const PlSizeSearch s = pl_size_begin(M, false);
            std::printf("%u %u %u %d\n", s.chosen, s.reached, s.probes, s.done ? 1 : 0);
        } else if (cmd == "A") {
            int32_t status = 0;
            uint64_t bytes = 0, max_bytes = 0;
            in >> status >> bytes >> max_bytes;
            if (!in) return 2;
            std::printf("%d\n", pl_size_accept(status, bytes, max_bytes) ? 1 : 0);
        } else if (cmd == "C") {
            pngloss_hip_size_target t{};
            int null_budgets = 0;
            in >> t.max_strength >> null_budgets;
            std::vector<uint32_t> w, h;
            std::vector<uint64_t> b;
            for (uint32_t a, c; in >> a >> c;) { uint64_t v = 0; in >> v; w.push_back(a); h.push_back(c); b.push_back(v); }
            t.max_bytes = null_budgets ? nullptr : b.data();
            std::printf("%d\n", pl_size_check(&t, w.size(), w.data(), h.data()));
        } else if (cmd == "G") {
            std::vector<PlSizeSearch> s;
            for (long v; in >> v;) {
                PlSizeSearch one = pl_size_begin(v < 0 ? 0 : (uint32_t)v, true);
                one.done = v < 0;
                s.push_back(one);
            }
            std::string out;
            for (const auto &g : pl_size_groups(s)) {
                out += (out.empty() ? "" : " ") + std::to_string(g.first) + ":";
                for (size_t k = 0; k < g.second.size(); k++) out += (k ? "," : "") + std::to_string(g.second[k]);
            }
            std::printf("%s\n", out.c_str());
        } else if (cmd == "L") {
            int host = 0, scan = 0;
            in >> host >> scan;
            std::vector<uint32_t> w, h;
            for (uint32_t a, b; in >> a >> b;) { w.push_back(a); h.push_back(b); }
            const PlTargetLayout lay = scan < 0 ? pl_target_layout(w, h, host != 0, 24, 32, 64) : pl_target_layout(w, h, host != 0, 24, 32, 64, 0, 0, scan);
            std::printf("%zu %zu %zu %zu %zu", lay.total, lay.moves, lay.jobs, lay.records, lay.flags);
            for (const PlTargetImage &m : lay.image)
                std::printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %u", m.orig, m.best, m.best_filters, m.img, m.filters, m.rows, m.ids, m.best_rows, m.best_ids, m.pitch);
            std::printf("\n");
        } else if (cmd == "R") {
            std::printf("%zu %zu %zu %zu\n", sizeof(PlSizeRecord), offsetof(PlSizeRecord, bytes), offsetof(PlSizeRecord, adler), offsetof(PlSizeRecord, kinds));
        } else return 2;
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

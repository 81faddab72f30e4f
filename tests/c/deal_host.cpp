/*
 * deal_host.cpp -- TEST INFRASTRUCTURE: the index bookkeeping of the multi-GPU wrapper and of the searches' host forms (pngloss_amd/csrc/pl_deal.h)
 * on the CPU.  Built with -fsanitize=address,undefined and run by tests/test_deal_host.py, which compares every line with a restatement of the
 * rule in Python.  Never shipped.
 *
 *   deal_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   S PARTS PIXELS_0 PIXELS_1 ...   pl_deal_owners -> owner_0 owner_1 ...
 *   D PARTS OWNER_0 OWNER_1 ...     pl_deal -> part:i,i,... for every part (empty ones too), then "|", then part.index per image
 *   G STRENGTH_0 STRENGTH_1 ...     pl_strength_groups -> strength:i,i,... per group
 *   F RC_0 RC_1 ...                 pl_fold_rc, one code after the other and the whole list at once -> the two answers
 */
#include "../../pngloss_amd/csrc/pl_deal.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

static std::string list_of(const std::vector<size_t> &v)
{
    std::string out;
    for (size_t k = 0; k < v.size(); k++) out += (k ? "," : "") + std::to_string(v[k]);
    return out;
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream in(line);
        std::string cmd, out;
        if (!(in >> cmd)) continue;
        if (cmd == "S") {
            int parts = 0;
            in >> parts;
            std::vector<uint64_t> pixels;
            for (uint64_t v; in >> v;) pixels.push_back(v);
            const std::vector<int> owner = pl_deal_owners(pixels, parts);
            if (owner.size() != pixels.size()) return 3;
            for (size_t i = 0; i < owner.size(); i++) out += (i ? " " : "") + std::to_string(owner[i]);
        } else if (cmd == "D") {
            int parts = 0;
            in >> parts;
            std::vector<int> owner;
            for (int v; in >> v;) { if (v < 0 || v >= parts) return 2; owner.push_back(v); }
            /* (as the dealer does: the owner array is never empty, its length is passed beside it) */
            const size_t n = owner.size();
            if (owner.empty()) owner.push_back(0);
            const PlDeal d = pl_deal(owner.data(), n, parts);
            if (d.where.size() != n) return 3;
            for (size_t p = 0; p < d.part.size(); p++) out += (p ? " " : "") + std::to_string(p) + ":" + list_of(d.part[p]);
            out += " |";
            for (const auto &w : d.where) out += " " + std::to_string(w.first) + "." + std::to_string(w.second);
        } else if (cmd == "G") {
            std::vector<uint32_t> strength;
            for (uint32_t v; in >> v;) strength.push_back(v);
            for (const auto &g : pl_strength_groups(strength)) out += (out.empty() ? "" : " ") + std::to_string(g.first) + ":" + list_of(g.second);
        } else if (cmd == "F") {
            std::vector<int> rcs;
            for (int v; in >> v;) rcs.push_back(v);
            int worst = PNGLOSS_SUCCESS;
            for (int rc : rcs) worst = pl_fold_rc(worst, rc);
            out = std::to_string(worst) + " " + std::to_string(pl_fold_rc(rcs));
        } else return 2;
        std::printf("%s\n", out.c_str());
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

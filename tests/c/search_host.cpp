/*
 * search_host.cpp -- TEST INFRASTRUCTURE: whole searches of pngloss_hip_optimize_batch_target and pngloss_hip_optimize_batch_size on the CPU, with
 * the bookkeeping of pngloss_amd/csrc/pl_search.h and a device made of tags.  Built with -fsanitize=address,undefined and run by
 * tests/test_search_host.py, which compares every line with the rules restated in Python (tests/util_target.py, tests/util_size.py).  Never shipped.
 *
 *   search_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   T COMMIT M IMAGE...            a target search below M over the images
 *   Z COMMIT STREAMS M IMAGE...    a size search (STREAMS 1: the caller wants the streams written; counts only with COMMIT)
 * IMAGE is W H FILTERS FAIL TABLE: width, height, 1 if the image has a filter array, the strength at which a probe comes back with a status other
 * than 0 (-1: none), and M + 1 characters '0' / '1': is a probe at strength s accepted.
 *   -> per image chosen/reached/probes/runs/failed/probe_1,probe_2,...   (reached of a target search: 1)
 *
 * The device: every region of every image (PlArenaRegion) holds a tag -- unset, the original, or the result of a strength.  A group at strength s
 * writes s into the image and its filters (size search: into rows and ids too); a move table is applied as ONE launch, every source read before any
 * destination is written.  The flow is that of pl_host.hip:target_search / size_search -- open, rounds of back / groups / measure / settle, close --
 * with the batches and measurements replaced by the tables.  On the way (exit code 3 and a message):
 *   1. when a probe of an image begins, the image holds the original
 *   2. no move reads an unset region; no table has two jobs with one destination, or a job whose destination is another job's source
 *   3. no table has more moves than the layout reserves (PLT_MOVES_PER_IMAGE, PLT_SIZE_MOVES_PER_IMAGE per image)
 *   4. with COMMIT every image that has pixels and did not fail ends holding the result of its chosen strength, in its filters too where it has
 *      them; what is kept is that strength's record; with STREAMS the region kept_in_stash names holds that strength's rows and ids.  Without
 *      COMMIT nothing is moved or run at the end
 *   5. a failed image keeps the failing probe's record, and that probe's result is in place
 */
#include "../../pngloss_amd/csrc/pl_search.h"

#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

namespace {
constexpr int UNSET = -2, ORIGINAL = -1;
constexpr int32_t FAILED_STATUS = 65;
constexpr uint32_t FLAG_TAG = 1000;

[[noreturn]] void broken(const char *what, size_t image, long detail)
{
    std::fprintf(stderr, "search_host: %s (image %zu, %ld)\n", what, image, detail);
    std::exit(3);
}

struct Image {
    uint32_t width = 0, height = 0, pitch = 0;
    bool filters = false;
    long fail_at = -1;
    std::string table;
    int tag[PLA_REGIONS];
    std::string seq;
    uint32_t ran = 0;
    bool pixels() const { return width && height; }
    uint64_t bytes(PlArenaRegion r) const { return pl_search_region_bytes(r, width, height, filters, pitch); }
};

struct Device {
    std::vector<Image> im;
    size_t reserve = 0;            /* moves per table */
    bool rows = false;             /* a group writes rows and ids */

    void move(const std::vector<PlSearchMove> &moves)
    {
        if (moves.size() > reserve) broken("a table is larger than the layout's room", moves.size(), (long)reserve);
        std::vector<PlSearchMove> jobs;
        for (const PlSearchMove &m : moves)
            if (im[m.image].bytes(m.src)) jobs.push_back(m);
        std::vector<int> read(jobs.size());
        for (size_t k = 0; k < jobs.size(); k++) {
            const PlSearchMove &m = jobs[k];
            if (im[m.image].bytes(m.src) != im[m.image].bytes(m.dst)) broken("a move between regions of two sizes", m.image, m.dst);
            read[k] = im[m.image].tag[m.src];
            if (read[k] == UNSET) broken("a move reads an unset region", m.image, m.src);
            for (size_t j = 0; j < jobs.size(); j++) {
                if (j != k && jobs[j].image == m.image && jobs[j].dst == m.dst) broken("two jobs of a table with one destination", m.image, m.dst);
                if (jobs[j].image == m.image && jobs[j].src == m.dst) broken("a job writes what another job of the table reads", m.image, m.dst);
            }
        }
        for (size_t k = 0; k < jobs.size(); k++) im[jobs[k].image].tag[jobs[k].dst] = read[k];
    }
    /* one batch: the result of image i, its record tagged with the strength */
    pngloss_hip_result run(uint32_t i, uint32_t strength, bool probe)
    {
        Image &m = im[i];
        if (m.pixels() && m.tag[PLA_IMAGE] != ORIGINAL) broken("a run begins on an image that does not hold its original", i, m.tag[PLA_IMAGE]);
        const PlArenaRegion wrote[] = { PLA_IMAGE, PLA_FILTERS, PLA_ROWS, PLA_IDS };
        for (int k = 0; k < (rows ? 4 : 2); k++)
            if (m.bytes(wrote[k])) m.tag[wrote[k]] = (int)strength;
        if (probe) m.seq += (m.seq.empty() ? "" : ",") + std::to_string(strength);
        m.ran++;
        return pngloss_hip_result{ m.fail_at == (long)strength ? FAILED_STATUS : 0, 4, strength, 0, 0 };
    }
    bool accepted(uint32_t i, uint32_t strength) const { return im[i].table[strength] == '1'; }
};

bool read_images(std::istringstream &in, uint32_t M, int scanlines, Device &dev)
{
    Image m;
    while (in >> m.width >> m.height) {
        int filters = 0;
        if (!(in >> filters >> m.fail_at >> m.table) || m.table.size() != (size_t)M + 1) return false;
        m.filters = filters != 0;
        for (int &t : m.tag) t = UNSET;
        if (m.pixels()) m.tag[PLA_IMAGE] = ORIGINAL;
        dev.im.push_back(m);
    }
    std::vector<uint32_t> w, h;
    for (const Image &one : dev.im) { w.push_back(one.width); h.push_back(one.height); }
    const PlTargetLayout lay = pl_target_layout(w, h, false, 24, 32, 64, 0, 0, scanlines);
    for (size_t i = 0; i < dev.im.size(); i++) dev.im[i].pitch = lay.image[i].pitch;
    dev.reserve = (scanlines ? PLT_SIZE_MOVES_PER_IMAGE : PLT_MOVES_PER_IMAGE) * dev.im.size();
    if ((lay.jobs - lay.moves) < 24 * dev.reserve) broken("the layout reserves less than the constants say", dev.im.size(), (long)(lay.jobs - lay.moves));
    dev.rows = scanlines != PLT_SCANLINES_OFF;
    return true;
}

/* assertions 4 and 5, and the answer line */
template <class Track>
void finish(const Device &dev, const std::vector<Track> &st, bool commit, const std::vector<uint32_t> &reached)
{
    std::string out;
    for (size_t i = 0; i < st.size(); i++) {
        const Track &s = st[i];
        const Image &m = dev.im[i];
        const int chosen = (int)s.search.chosen;
        if (!s.search.done) broken("the search ended with an image still searching", i, 0);
        if (s.runs != m.ran) broken("runs is not the number of batches the image was in", i, s.runs);
        if (s.search.failed) {
            if (s.kept.result.status != FAILED_STATUS || (int)s.kept.result.unique_symbols != chosen) broken("a failed image does not keep the failing probe", i, chosen);
            if (m.pixels() && m.tag[PLA_IMAGE] != chosen) broken("a failed image does not hold the failing probe's result", i, m.tag[PLA_IMAGE]);
        } else if (commit && m.pixels()) {
            if (m.tag[PLA_IMAGE] != chosen) broken("the image does not end with its chosen strength's result", i, m.tag[PLA_IMAGE]);
            if (m.bytes(PLA_FILTERS) && m.tag[PLA_FILTERS] != chosen) broken("the filters do not end with the chosen strength's", i, m.tag[PLA_FILTERS]);
            if (s.kept.result.status != 0 || (int)s.kept.result.unique_symbols != chosen) broken("what is kept is not the chosen strength's record", i, s.kept.result.unique_symbols);
        }
        out += (i ? " " : "") + std::to_string(chosen) + "/" + std::to_string(reached[i]) + "/" + std::to_string(s.search.probes) + "/" +
               std::to_string(s.runs) + "/" + (s.search.failed ? "1" : "0") + "/" + m.seq;
    }
    std::printf("%s\n", out.c_str());
}

void target_search(Device &dev, uint32_t M, bool commit)
{
    const size_t n = dev.im.size();
    const pngloss_hip_target2 t = { 0.0, 1, M, 0.0 };               /* accepted: no channel error above 1 */
    std::vector<PlTargetTrack> st(n);
    for (size_t i = 0; i < n; i++) st[i].search = pl_target_begin(M);
    auto run_group = [&](uint32_t strength, const std::vector<uint32_t> &who, bool probe) {
        for (uint32_t i : who) pl_search_ran(st[i], strength, dev.run(i, strength, probe));
    };
    auto measure = [&](const std::vector<uint32_t> &who) {
        for (uint32_t i : who) {
            const uint32_t strength = (uint32_t)st[i].in_place;
            pngloss_hip_distortion rec{};
            rec.pixels = (uint64_t)dev.im[i].width * dev.im[i].height;
            rec.changed_pixels = strength;
            rec.max_abs[0] = dev.accepted(i, strength) ? 1 : 2;
            st[i].last.rec = rec;
        }
    };
    dev.move(pl_search_open(n));
    for (;;) {
        const PlSearchRound round = pl_search_round(st);
        if (round.groups.empty()) break;
        dev.move(round.back);
        for (const auto &g : round.groups) run_group(g.first, g.second, true);
        measure(round.probed);
        dev.move(pl_target_settle(st, round.probed, t));
    }
    const PlTargetClose close = pl_target_close(st, commit);
    if (!commit && !close.fin.empty()) broken("a search that does not commit moves at the end", 0, (long)close.fin.size());
    dev.move(close.fin);
    if (commit && !close.zero.empty()) {
        run_group(0, close.zero, false);
        measure(close.zero);
        pl_target_reran(st, close.zero);
    }
    for (size_t i = 0; i < n; i++)
        if (!st[i].search.failed && st[i].kept.rec.changed_pixels != st[i].kept.result.unique_symbols) broken("the kept record and the kept result are of two probes", i, (long)st[i].kept.rec.changed_pixels);
    finish(dev, st, commit, std::vector<uint32_t>(n, 1));
}

void size_search(Device &dev, uint32_t M, bool commit, bool want_streams)
{
    const size_t n = dev.im.size();
    const std::vector<uint64_t> budget(n, 100);                      /* accepted: a stream of 100 bytes at most */
    std::vector<PlSizeTrack> st(n);
    for (size_t i = 0; i < n; i++) st[i].search = pl_size_begin(M, dev.im[i].pixels());
    dev.move(pl_search_open(n));
    for (;;) {
        const PlSearchRound round = pl_search_round(st);
        if (round.groups.empty()) break;
        dev.move(round.back);
        for (const auto &g : round.groups)
            for (uint32_t i : g.second) {
                pl_search_ran(st[i], g.first, dev.run(i, g.first, true));
                st[i].last.flags = st[i].last.result.status == 0 ? FLAG_TAG + g.first : 0;
            }
        for (uint32_t i : round.probed)
            if (st[i].last.result.status == 0) {
                const uint32_t strength = (uint32_t)st[i].in_place;
                st[i].last.size = PlSizeRecord{ dev.accepted(i, strength) ? 100u : 101u, strength, { 0, 0, 0 } };
            }
        dev.move(pl_size_settle(st, round.probed, budget.data(), want_streams));
    }
    const std::vector<PlSearchMove> fin = pl_size_close(st, commit);
    if (!commit && !fin.empty()) broken("a search that does not commit moves at the end", 0, (long)fin.size());
    dev.move(fin);
    for (size_t i = 0; i < n; i++) {
        const PlSizeTrack &s = st[i];
        const Image &m = dev.im[i];
        if (s.search.failed) {
            if (s.kept.flags != 0 || s.kept.size.bytes != 0 || s.search.reached != 0) broken("a failed image reports a stream", i, (long)s.kept.size.bytes);
            continue;
        }
        if (!m.pixels()) continue;
        if (s.kept.flags != FLAG_TAG + s.search.chosen || s.kept.size.adler != s.search.chosen) broken("the kept flags or size are not the chosen strength's", i, s.kept.flags);
        if ((s.kept.size.bytes <= 100) != (s.search.reached != 0)) broken("reached does not say whether the kept stream fits", i, s.search.reached);
        if (want_streams) {
            const int chosen = (int)s.search.chosen;
            if (m.tag[s.kept_in_stash ? PLA_BEST_ROWS : PLA_ROWS] != chosen || m.tag[s.kept_in_stash ? PLA_BEST_IDS : PLA_IDS] != chosen)
                broken("the region kept_in_stash names does not hold the chosen strength's scanlines", i, s.kept_in_stash);
        } else if (s.kept_in_stash) broken("kept_in_stash without streams", i, 0);
    }
    std::vector<uint32_t> reached(n);
    for (size_t i = 0; i < n; i++) reached[i] = st[i].search.reached;
    finish(dev, st, commit, reached);
}
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
        int commit = 0, streams = 0;
        uint32_t M = 0;
        Device dev;
        if (cmd == "T") {
            if (!(in >> commit >> M) || M > 255 || !read_images(in, M, PLT_SCANLINES_OFF, dev)) return 2;
            target_search(dev, M, commit != 0);
        } else if (cmd == "Z") {
            if (!(in >> commit >> streams >> M) || M > 255 || !read_images(in, M, streams ? PLT_SCANLINES_PROBE_AND_BEST : PLT_SCANLINES_PROBE, dev)) return 2;
            size_search(dev, M, commit != 0, commit != 0 && streams != 0);
        } else return 2;
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

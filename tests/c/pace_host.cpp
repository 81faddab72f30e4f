/*
 * pace_host.cpp -- TEST INFRASTRUCTURE: the launch loop of the segment engine (pngloss_amd/csrc/pl_host.hip:seg_worker_main) on the CPU, with the decisions of
 * pngloss_amd/csrc/pl_seg_pace.h and a scripted device.  Built with -fsanitize=address,undefined and run by tests/test_pace_host.py, which compares every
 * answer with the rules restated in Python.  Never shipped.
 *
 *   pace_host COMMANDS
 * COMMANDS is text, one command per line, one answer line each:
 *   W                                      -> the number of host-visible words, then per group of SEG_MAX_GROUPS its done:attempt:break word
 *   P NGROUPS MAX_ATTEMPTS T0 {N SEEDS}.. NPOLLS {T_POLL T_IDLE {DONE ATTEMPT BREAKS}..}..
 *        a batch of NGROUPS launch groups (N images, SEEDS 0 / 1 each) begun at time T0 (nanoseconds), then NPOLLS passes of the loop: the clock reads T_POLL
 *        at the top of the pass and T_IDLE behind it, and the device shows every group's three words
 *     -> per pass one token per group polled -- F finished, B busy, R runaway, L<attempt>:<seeds> a launch -- and one for the pass: + something was launched,
 *        Y yield, Z sleep, S stalled, D every group finished; the loop ends at D, R, S or the end of the script.  Then "|", the attempts the batch reports,
 *        the look-ahead statistics sum,count,least,low and every host-visible word as the loop leaves it (after R and S: released)
 *   C HOOK SLOT CPU..                      -> the CPU the launch thread pins itself to out of that affinity set, or -1
 *   Q OK DISTINCT SYNC THIRD DEFAULT KNOWN PRIO SEG_PRIO   -> 1 if the caller's stream gets a device-side wait
 */
#include "../../pngloss_amd/csrc/pl_seg_pace.h"

#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

namespace {

bool run(std::istringstream &in)
{
    int ngroups = 0, npolls = 0;
    long max_attempts = 0;
    int64_t t0 = 0;
    if (!(in >> ngroups >> max_attempts >> t0) || ngroups < 1 || ngroups > SEG_MAX_GROUPS) return false;
    PlSegPace pace = pl_seg_pace_begin(ngroups, max_attempts, t0);
    size_t n[SEG_MAX_GROUPS] = {};
    for (int g = 0; g < ngroups; g++) {
        int seeds = 0;
        if (!(in >> n[g] >> seeds)) return false;
        pl_seg_pace_group(pace, g, n[g], seeds != 0);
    }
    if (!(in >> npolls)) return false;
    volatile uint32_t words[PL_SEG_WORDS] = {};
    bool failed = false, all_done = false;
    for (int k = 0; k < npolls && !failed && !all_done; k++) {
        int64_t t_poll = 0, t_idle = 0;
        if (!(in >> t_poll >> t_idle)) return false;
        for (int g = 0; g < ngroups; g++) {
            uint32_t done = 0, attempt = 0, breaks = 0;
            if (!(in >> done >> attempt >> breaks)) return false;
            words[pl_seg_done_word(g)] = done; words[pl_seg_attempt_word(g)] = attempt; words[pl_seg_break_word(g)] = breaks;
        }
        /* (the pass of seg_worker_main, its calls replaced by printing) */
        bool any_launched = false;
        all_done = true;
        for (int g = 0; g < ngroups && !failed; g++) {
            const PlSegStep step = pl_seg_pace_poll(pace, g, pl_seg_words_read(words, g), t_poll);
            if (step == PlSegStep::Finished) { std::printf("F "); continue; }
            all_done = false;
            if (step == PlSegStep::Busy) { std::printf("B "); continue; }
            if (step == PlSegStep::Runaway) { std::printf("R "); failed = true; break; }
            std::printf("L%ld:%d ", pace.g[g].launched, pace.g[g].seeds ? 1 : 0);
            pl_seg_pace_launched(pace, g);
            any_launched = true;
        }
        if (failed) break;
        if (all_done) { std::printf("D "); break; }
        if (any_launched) { std::printf("+ "); continue; }
        switch (pl_seg_pace_idle(pace, t_idle)) {
        case PlSegIdle::Stalled: std::printf("S "); failed = true; break;
        case PlSegIdle::Yield: std::printf("Y "); break;
        case PlSegIdle::Sleep: std::printf("Z "); break;
        }
    }
    if (failed)
        for (int g = 0; g < ngroups; g++) pl_seg_words_release(words, g, n[g]);
    std::printf("| %ld %ld,%ld,%ld,%ld", pl_seg_pace_attempts(pace), pace.lead_sum, pace.lead_n, pace.lead_min, pace.lead_low);
    for (int q = 0; q < PL_SEG_WORDS; q++) std::printf(" %u", words[q]);
    std::printf("\n");
    return true;
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
        if (cmd == "W") {
            std::printf("%d", PL_SEG_WORDS);
            for (int g = 0; g < SEG_MAX_GROUPS; g++) std::printf(" %d:%d:%d", pl_seg_done_word(g), pl_seg_attempt_word(g), pl_seg_break_word(g));
            std::printf("\n");
        } else if (cmd == "P") {
            if (!run(in)) return 2;
        } else if (cmd == "C") {
            int hook = 0, slot = 0, c = 0;
            if (!(in >> hook >> slot)) return 2;
            std::vector<int> cpus;
            while (in >> c) cpus.push_back(c);
            std::printf("%d\n", pl_seg_pin_cpu(cpus.data(), cpus.size(), slot, hook));
        } else if (cmd == "Q") {
            int v[8] = {};
            for (int &x : v) if (!(in >> x)) return 2;
            std::printf("%d\n", pl_seg_wait_on_device(v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6], v[7]) ? 1 : 0);
        } else return 2;
    }
    std::free(line);
    std::fclose(f);
    return 0;
}

"""The launch loop of the segment engine (pngloss_amd/csrc/pl_seg_pace.h: the host-visible words, throttle, runaway bound, the switch away from seeds, look-ahead
statistics, stall watchdog, back-off, error release, the launch thread's CPU and the caller's device-side wait) driven by a scripted device through
tests/c/pace_host.cpp, under the sanitizers.  Every expected answer comes from the rules as seg_worker_main and run_seg_engine had them inline in pl_host.hip
before the header existed, restated here in Python (Loop, py_pin_cpu, py_wait below: written from that code, not from the header)."""
import random

import pytest

from tests import util_size as S

MAX_GROUPS = 8
SEC = 1000 ** 3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("pace_host")
    return S.build_pace_host(d), d


class Loop:
    """seg_worker_main's loop: one pass() per trip, the launches and waits as tokens (tests/c/pace_host.cpp says which)"""

    def __init__(self, max_attempts, t0, groups):
        self.n = [n for n, _ in groups]
        self.seeds = [bool(s) for _, s in groups]
        self.max_attempts, self.t0 = max_attempts, t0
        self.launched = [0] * len(groups)
        self.seen = [0] * len(groups)
        self.t_last = t0
        self.idle = 0
        self.lead_sum, self.lead_n, self.lead_min, self.lead_low = 0, 0, 1 << 30, 0
        self.words = [0] * (4 * MAX_GROUPS)
        self.tokens = []
        self.over = False

    def pass_(self, t_poll, t_idle, words):
        """words: (done, attempt, breaks) per group"""
        assert not self.over
        all_done, any_launched, rc = True, False, 0
        for g, (done, at, breaks) in enumerate(words):
            self.words[2 * g], self.words[2 * g + 1], self.words[2 * MAX_GROUPS + g] = done, at, breaks
        for g, (done, at, breaks) in enumerate(words):
            if done >= self.n[g]:
                self.tokens.append("F")
                continue
            all_done = False
            if at != self.seen[g]:
                self.seen[g], self.t_last, self.idle = at, t_poll, 0
            if self.launched[g] - at > 32:
                self.tokens.append("B")
                continue
            if self.launched[g] > self.max_attempts:
                self.tokens.append("R")
                rc = 1
                break
            if self.seeds[g] and breaks * 25 > at * self.n[g] + 400:       # (64-bit in the loop: Python's integers do not wrap)
                self.seeds[g] = False
            if self.launched[g] >= 64:
                lead = self.launched[g] - at
                self.lead_sum += lead
                self.lead_n += 1
                self.lead_min = min(self.lead_min, lead)
                self.lead_low += lead <= 2
            self.tokens.append("L%d:%d" % (self.launched[g], self.seeds[g]))
            self.launched[g] += 1
            any_launched = True
        if rc == 0 and all_done:
            self.tokens.append("D")
            self.over = True
        elif rc == 0 and any_launched:
            self.tokens.append("+")
        elif rc == 0:
            if t_idle - self.t_last > 20 * SEC:
                self.tokens.append("S")
                rc = 1
            else:
                self.idle += 1
                self.tokens.append("Y" if self.idle < 4 else "Z")
        if rc:
            for g in range(len(self.n)):
                self.words[2 * g] = self.n[g]
            self.over = True

    def answer(self):
        return " ".join(self.tokens + ["|", str(max(self.launched)), "%d,%d,%d,%d" % (self.lead_sum, self.lead_n, self.lead_min, self.lead_low)] + [str(w) for w in self.words])


def both(host, max_attempts, t0, groups, polls):
    """the script through the harness and through the restatement: (tokens, tail) after checking that the two agree"""
    exe, d = host
    loop = Loop(max_attempts, t0, groups)
    for t_poll, t_idle, words in polls:
        if loop.over:
            break
        loop.pass_(t_poll, t_idle, words)
    cmd = "P %d %d %d %s %d %s" % (len(groups), max_attempts, t0, " ".join("%d %d" % (n, s) for n, s in groups), len(polls),
                                   " ".join("%d %d %s" % (tp, ti, " ".join("%d %d %d" % w for w in words)) for tp, ti, words in polls))
    (line,) = S.run_host(exe, d, [cmd])
    assert " ".join(line.split()) == loop.answer()
    head, tail = line.split("|")
    return head.split(), tail.split()


def test_the_host_visible_words(host):
    """[2g] images of group g that are finished, [2g + 1] the attempt its first image works on, [2 * SEG_MAX_GROUPS + g] rows the chain kernel broke off; 16 bytes per group"""
    exe, d = host
    (line,) = S.run_host(exe, d, ["W"])
    assert line.split() == [str(16 * MAX_GROUPS // 4)] + ["%d:%d:%d" % (2 * g, 2 * g + 1, 2 * MAX_GROUPS + g) for g in range(MAX_GROUPS)]


def test_throttle_launches_at_32_ahead_and_waits_at_33(host):
    polls = [(k, k, [(0, 0, 0)]) for k in range(35)] + [(40, 40, [(0, 1, 0)]), (41, 41, [(0, 1, 0)])]
    tok, _ = both(host, 10 ** 6, 0, [(1, 0)], polls)
    runs = [t for t in tok if t not in "+YZ"]
    assert runs == ["L%d:0" % k for k in range(33)] + ["B", "B", "L33:0", "B"]      # launched - at == 32: launch; 33: busy; the device moves on by one: one more


def test_runaway_one_past_the_bound(host):
    polls = [(k, k, [(0, k, 0), (0, 0, 0)]) for k in range(10)]
    tok, tail = both(host, 5, 0, [(2, 0), (7, 0)], polls)
    assert [t for t in tok if t.startswith("L")][-2:] == ["L5:0", "L5:0"] and tok[-1] == "R" and tok.count("R") == 1      # a launch at launched == max_attempts, runaway one later
    assert tail[0] == "6"
    words = [int(w) for w in tail[2:]]
    assert words[0] == 2 and words[2] == 7 and words[1] == 6 and words[3] == 0 and not any(words[4:])    # released: every group's image count in its finished word


def test_seeds_switch_is_strict_sticks_and_does_not_wrap(host):
    n, at = 3, 100
    polls = [(0, 0, [(0, at, 28)]), (1, 1, [(0, at, 29)]), (2, 2, [(0, at, 0)])]       # 28 * 25 == 100 * 3 + 400
    tok, _ = both(host, 10 ** 6, 0, [(n, 1)], polls)
    assert [t for t in tok if t.startswith("L")] == ["L0:1", "L1:0", "L2:0"]
    # attempt * images beyond 2^32: 2.5e9 is below 6e9 + 400 -- and above what is left of it in 32 bits
    at, breaks = 2 * 10 ** 9, 10 ** 8
    assert breaks * 25 < 2 ** 32 and at * n > 2 ** 32 and breaks * 25 > (at * n + 400) % 2 ** 32
    tok, _ = both(host, 10 ** 6, 0, [(n, 1)], [(0, 0, [(0, at, breaks)]), (1, 1, [(0, at, (at * n + 400) // 25 + 1)])])
    assert [t for t in tok if t.startswith("L")] == ["L0:1", "L1:0"]
    # a group that begins without seeds never gets them
    tok, _ = both(host, 10 ** 6, 0, [(n, 0)], [(0, 0, [(0, 5, 0)])])
    assert tok[0] == "L0:0"


def test_a_finished_group_is_skipped_while_another_goes_on(host):
    polls = [(k, k, [(4, 0, 0), (k // 2, k, 0)]) for k in range(5)]
    tok, tail = both(host, 100, 0, [(4, 0), (2, 0)], polls)
    assert tok == ["F", "L0:0", "+", "F", "L1:0", "+", "F", "L2:0", "+", "F", "L3:0", "+", "F", "F", "D"]
    assert tail[0] == "4"
    assert [int(w) for w in tail[2:6]] == [4, 0, 2, 4]      # not released: the words as the device left them


def test_statistics_begin_with_the_65th_launch(host):
    polls = [(k, k, [(0, max(0, k - 1), 0)]) for k in range(64)]
    _, tail = both(host, 1000, 0, [(1, 0)], polls)
    assert tail[1] == "0,0,%d,0" % (1 << 30)
    polls += [(64, 64, [(0, 60, 0)]), (65, 65, [(0, 63, 0)]), (66, 66, [(0, 35, 0)])]
    _, tail = both(host, 1000, 0, [(1, 0)], polls)
    assert tail[1] == "%d,3,2,1" % (4 + 2 + 31)


def test_stall_after_more_than_twenty_seconds_without_progress(host):
    busy = [(0, 0, [(0, 0, 0)])] * 33          # 33 attempts queued, the device at 0: nothing to launch from here on
    tok, tail = both(host, 100, 7, [(1, 0)], busy + [(8, 20 * SEC + 7, [(0, 0, 0)]), (9, 20 * SEC + 8, [(0, 0, 0)])])
    assert tok[-4:] == ["B", "Y", "B", "S"]
    assert tail[2] == "1"                                                       # released
    # progress in ANY unfinished group restarts the clock; a finished group's word does not
    groups = [(1, 0), (1, 0), (1, 0)]
    still = [(0, 0, 0), (0, 0, 0), (1, 0, 0)]
    moved = [(0, 0, 0), (0, 1, 0), (1, 0, 0)]
    late = [(0, 0, 0), (0, 1, 0), (1, 9, 0)]
    polls = [(0, 0, still)] * 33 + [(15 * SEC, 15 * SEC, moved)] + [(16 * SEC, 16 * SEC, moved)] * 2 + [(30 * SEC, 35 * SEC, late), (35 * SEC, 35 * SEC + 1, late)]
    tok, _ = both(host, 100, 0, groups, polls)
    assert tok[-8:] == ["B", "B", "F", "Y", "B", "B", "F", "S"] and tok.count("S") == 1


def test_back_off_yields_three_times_then_sleeps(host):
    busy = [(0, 0, [(0, 0, 0)])] * 33
    tok, _ = both(host, 100, 0, [(1, 0)], busy + [(1, 1, [(0, 0, 0)])] * 6 + [(2, 2, [(0, 1, 0)])] + [(3, 3, [(0, 1, 0)])] * 2)
    assert [t for t in tok if t in "YZ+"][33:] == ["Y", "Y", "Y", "Z", "Z", "Z", "+", "Y", "Y"]      # (progress starts the back-off over)


def py_pin_cpu(cpus, slot, hook):
    if hook != 0:
        want = 2 * slot + 1
        if len(cpus) >= 4 and want < len(cpus):
            return cpus[want]
    return -1


def test_the_cpu_of_the_launch_thread(host):
    exe, d = host
    cases = [(-1, 0, [4, 5, 6]), (-1, 0, [4, 5, 6, 9]), (-1, 1, [4, 5, 6, 9]), (-1, 2, [4, 5, 6, 9, 11]), (1, 2, [4, 5, 6, 9, 11, 12]), (0, 0, [4, 5, 6, 9]), (-1, 0, []),
             (1, 7, list(range(0, 32, 2)))]
    got = S.run_host(exe, d, ["C %d %d %s" % (hook, slot, " ".join(map(str, cpus))) for hook, slot, cpus in cases])
    assert [int(x) for x in got] == [py_pin_cpu(cpus, slot, hook) for hook, slot, cpus in cases] == [-1, 5, 9, -1, 12, -1, -1, 30]


def py_wait(ok, distinct, sync, third, default_stream, known, prio, seg_prio):
    waiting = ok and distinct and not sync and not third
    if waiting and not default_stream:
        if not known or prio == seg_prio:
            waiting = False
    return int(bool(waiting))


def test_the_callers_stream_waits_on_the_device(host):
    exe, d = host
    good = (1, 1, 0, 0, 0, 1, 0, -1)
    cases = [good, (0,) + good[1:], (1, 0) + good[2:], (1, 1, 1) + good[3:], (1, 1, 0, 1) + good[4:], good[:5] + (0, 0, -1), good[:6] + (-1, -1),
             (1, 1, 0, 0, 1, 0, -1, -1), (0, 1, 0, 0, 1, 1, 0, -1)]      # (the default stream's priority is not asked for)
    got = S.run_host(exe, d, ["Q " + " ".join(map(str, c)) for c in cases])
    assert [int(x) for x in got] == [py_wait(*c) for c in cases] == [1, 0, 0, 0, 0, 0, 0, 1, 0]


def test_random_scripts(host):
    """a few thousand passes over devices that run ahead, fall behind, break rows, finish and hang"""
    rng = random.Random(7)
    exe, d = host
    cmds, want, passes = [], [], 0
    for _ in range(60):
        groups = [(rng.randint(1, 5), rng.randint(0, 1)) for _ in range(rng.choice([1, 1, 2, 2, 3, 4, MAX_GROUPS]))]
        max_attempts = rng.choice([50, 10 ** 6, 10 ** 6])
        t = rng.randint(0, 10 ** 12)
        loop = Loop(max_attempts, t, groups)
        at, done, breaks = [0] * len(groups), [0] * len(groups), [0] * len(groups)
        polls = []
        for _ in range(rng.randint(40, 250)):
            t_poll = t + rng.randint(0, 10 ** 5)
            t = t_idle = t_poll + rng.choice([0, 50, 10 ** 5, 10 ** 5, 7 * SEC, 21 * SEC] if rng.random() < 0.05 else [10, 200])
            for g in range(len(groups)):
                r = rng.random()
                if r < 0.25:
                    at[g] = min(loop.launched[g], at[g] + rng.randint(0, 2))
                elif r < 0.26:
                    at[g] = rng.randint(0, 2 ** 32 - 1)           # (a word the loop cannot explain: it must still answer as the rule says)
                if rng.random() < 0.1:
                    breaks[g] += rng.randint(0, 40)
                if rng.random() < 0.03:
                    done[g] = min(groups[g][0], done[g] + 1) if rng.random() < 0.8 else groups[g][0] + 1
            words = [(done[g], at[g], breaks[g]) for g in range(len(groups))]
            polls.append((t_poll, t_idle, words))
            loop.pass_(t_poll, t_idle, words)
            passes += 1
            if loop.over:
                break
        cmds.append("P %d %d %d %s %d %s" % (len(groups), max_attempts, loop.t0, " ".join("%d %d" % gs for gs in groups), len(polls),
                                             " ".join("%d %d %s" % (tp, ti, " ".join("%d %d %d" % w for w in ws)) for tp, ti, ws in polls)))
        want.append(loop.answer())
    assert passes >= 2000
    got = S.run_host(exe, d, cmds)
    assert [" ".join(line.split()) for line in got] == want
    joined = " ".join(want)
    assert all(tok in joined for tok in (" B ", " R ", " S ", " D ", " Z ", ":1 ", ":0 "))      # the scripts reach every answer

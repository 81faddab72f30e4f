"""CPU tests of pngloss_amd/csrc/pl_search.h (no GPU): the bookkeeping of the target search and of the size search -- what is kept, which arena
regions are copied where -- driven through whole searches on a device made of tags (tests/c/search_host.cpp, under the sanitizers).  The harness
itself asserts what the copies have to keep true (every probe starts from the original, well-formed move tables within the layout's room, the
chosen strength's result in place at the end, a failed image keeps its failing probe); this file compares what it prints -- chosen strength, probe
sequence, probes, runs, reached -- with the rules restated in tests/util_target.py and tests/util_size.py."""
import itertools

import numpy as np
import pytest

from tests import util_size as S
from tests import util_target as T

#: (commit, streams) of a size search; streams count only with commit
SIZE_MODES = [(0, 0), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("search_host")
    return S.build_search_host(d), d


def _table(bits):
    return "".join("1" if b else "0" for b in bits)


class _Failed(Exception):
    pass


def _asked(search, m, table, fail):
    """the probes of search(m, accepted) on a table, up to and including one at strength `fail`: (its return value or None, probe sequence)"""
    seq = []

    def accepted(s):
        seq.append(s)
        if s == fail:
            raise _Failed()
        return table[s]

    try:
        return search(m, accepted), seq
    except _Failed:
        return None, seq


def want_target(m, img, commit):
    """chosen/reached/probes/runs/failed/sequence of one image of a target search: an image without pixels is accepted whatever the table says; an
    image with no accepted probe is run once more, at 0, when the search commits"""
    w, h, _, fail, table = img
    if not w * h:
        table = [True] * (m + 1)
    got, seq = _asked(T.py_search, m, table, fail)
    if got is None:
        return (fail, 1, len(seq), len(seq), 1, seq)
    chosen = got[0]
    assert got[1] == seq
    rerun = bool(commit) and not any(table[s] for s in seq) and seq[-1] != 0
    return (chosen, 1, len(seq), len(seq) + rerun, 0, seq)


def want_size(m, img):
    w, h, _, fail, table = img
    if not w * h:
        return (0, 1, 0, 0, 0, [])
    got, seq = _asked(S.py_search, m, table, fail)
    if got is None:
        return (fail, 0, len(seq), len(seq), 1, seq)
    assert got[2] == seq
    return (got[0], got[1], len(seq), len(seq), 0, seq)


def _image(img):
    w, h, filt, fail, table = img
    return "%d %d %d %d %s" % (w, h, filt, fail, _table(table))


def _parse(line):
    out = []
    for item in line.split():
        f = item.split("/")
        out.append(tuple(int(x) for x in f[:5]) + ([int(x) for x in f[5].split(",")] if f[5] else [],))
    return out


def _check(harness, searches):
    """searches: (M, [image, ...]); each runs as a target search with and without commit and as a size search in every mode"""
    exe, d = harness
    cmds, want = [], []
    for m, images in searches:
        flat = " ".join(_image(i) for i in images)
        for commit in (0, 1):
            cmds.append("T %d %d %s" % (commit, m, flat))
            want.append([want_target(m, i, commit) for i in images])
        for commit, streams in SIZE_MODES:
            cmds.append("Z %d %d %d %s" % (commit, streams, m, flat))
            want.append([want_size(m, i) for i in images])
    got = S.run_host(exe, d, cmds)
    for cmd, line, w in zip(cmds, got, want):
        assert _parse(line) == w, cmd
    return want


def test_every_table_up_to_ten_one_image_each(harness):
    searches = [(m, [(7, 3, 1, -1, bits)]) for m in range(11) for bits in itertools.product((False, True), repeat=m + 1)]
    want = _check(harness, searches)
    # every way a search can end is among them: the last probe accepted, an earlier one kept, nothing accepted (target), M refused (size)
    target = [w[0] for w in want[1::5]]
    assert any(t[0] == t[5][-1] for t in target) and any(0 < t[0] != t[5][-1] for t in target) and any(t[3] == t[2] + 1 for t in target)
    size = [w[0] for w in want[4::5]]
    assert any(s[1] == 0 for s in size) and any(s[1] == 1 and s[0] != s[5][-1] for s in size) and any(s[0] == 0 for s in size)


def test_random_tables_at_19_40_and_255(harness):
    rng = np.random.default_rng(23)
    _check(harness, [(m, [(33, 5, int(rng.integers(0, 2)), -1, list(rng.random(m + 1) < rng.random()))]) for m in (19, 40, 255) for _ in range(60)])


def _batch(rng, m, n):
    """n images with tables of their own; among them one without pixels, one without a filter array, one whose probe fails at M and one whose
    probe fails at a strength in the middle of its sequence -- under either rule, so the fail strength is the second probe of both"""
    images = []
    for k in range(n):
        table = list(rng.random(m + 1) < rng.random())
        images.append([int(rng.integers(1, 140)), int(rng.integers(1, 20)), 1, -1, table])
    images[0][:2] = (0, 5) if rng.random() < 0.5 else (0, 0)
    images[1][2] = 0
    images[2][3] = m
    if m >= 3:
        # M refused by the target rule probes M / 2 second, M accepted by the size rule probes (M - 1) / 2 second: fail one image of each kind
        images[3][3], images[3][4][m] = m // 2, False
        images[4][3], images[4][4][m] = (m - 1) // 2, True
    order = rng.permutation(n)
    return m, [tuple(images[i]) for i in order]


def test_batches_share_their_tables(harness):
    rng = np.random.default_rng(29)
    searches = [_batch(rng, m, int(rng.integers(6, 9))) for m in (19, 40, 255, 5, 1, 0) for _ in range(8)]
    want = _check(harness, searches)
    failed_in_the_middle = [w for per in want for w in per if w[4] == 1 and w[2] > 1]
    assert failed_in_the_middle and any(w[4] == 1 and w[2] == 1 for per in want for w in per)


def test_the_non_monotone_cases_of_the_gpu_tests(harness):
    """cases 4 and 5 of util_target.CASES as tables: 11 and 12 refused between accepted neighbours; 15 accepted above a refused 9"""
    (_, m4, _, _, chosen4, seq4), (_, m5, _, _, chosen5, seq5) = T.CASES[3], T.CASES[4]
    t4 = [s <= 10 or 13 <= s <= 30 for s in range(m4 + 1)]
    t5 = [s <= 8 or s == 15 for s in range(m5 + 1)]
    assert m4 == m5 == 40 and T.py_search(m4, lambda s: t4[s]) == (chosen4, seq4) and T.py_search(m5, lambda s: t5[s]) == (chosen5, seq5)
    images = [(130, 6, 1, -1, t4), (64, 8, 1, -1, t5), (130, 6, 0, -1, t5), (64, 8, 1, -1, t4)]
    want = _check(harness, [(40, images)])
    assert [w[0] for w in want[1]] == [30, 8, 8, 30] and want[1][0][5] == seq4 and want[1][1][5] == seq5

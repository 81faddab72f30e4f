"""CPU tests of pngloss_amd/csrc/pl_deal.h (no GPU): the split of a batch over the contexts of a node, the deal that follows from it, the groups of a
searched batch by chosen strength and the fold of return codes, run on the CPU under the sanitizers (tests/c/deal_host.cpp) against the rules
restated here in a few lines of Python."""
import itertools

import numpy as np
import pytest

from pngloss_amd import lib as L
from pngloss_amd import shard
from tests import util_size as S

OK, ABORT, HIP, BAD = L.PNGLOSS_SUCCESS, L.PNGLOSS_INTERNAL_ABORT, L.PNGLOSS_HIP_ERROR, L.PNGLOSS_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("deal_host")
    return S.build_deal_host(d), d


def _ints(text):
    return [int(x) for x in text.split()]


def _lists(text):
    """'3:0,2 7:1' -> [(3, [0, 2]), (7, [1])]"""
    return [(int(k), [int(i) for i in v.split(",")] if v else []) for k, v in (item.split(":") for item in text.split())]


def _py_owners(pixels, parts):
    own = [None] * len(pixels)
    for r, items in enumerate(shard.lpt_partition(pixels, max(parts, 1))):
        for i in items:
            own[i] = r
    return own


def test_split_is_the_python_split(harness):
    exe, d = harness
    rng = np.random.default_rng(5)
    sizes = [[], [7], [3, 9], [5, 5, 5, 5], [640 * 480] * 11, [0, 0, 0], [12, 0, 7, 0, 0, 12, 1], [0, 100, 0, 100, 50, 50, 0],
             [int(v) for v in rng.integers(0, 4096 * 4096, 300)], [int(v) for v in rng.integers(0, 4, 257)]]
    cases = [(px, parts) for px in sizes for parts in (1, 2, 3, 8)]
    got = S.run_host(exe, d, ["S %d %s" % (parts, " ".join(map(str, px))) for px, parts in cases])
    for (px, parts), line in zip(cases, got):
        assert _ints(line) == _py_owners(px, parts), (px[:12], parts)
    assert any(len(px) and len(px) < parts for px, parts in cases)               # fewer images than parts: the parts behind stay empty
    # parts below 1 count as 1
    assert S.run_host(exe, d, ["S 0 4 9 1", "S -3 4 9 1", "S 1 4 9 1"]) == ["0 0 0"] * 3


def test_deal_gives_every_image_one_place(harness):
    exe, d = harness
    rng = np.random.default_rng(6)
    cases = [(1, []), (2, []), (3, [2]), (2, [0, 0, 0]), (8, [7, 0, 7, 3]), (3, [int(v) for v in rng.integers(0, 3, 200)]),
             (8, _py_owners([int(v) for v in rng.integers(0, 1 << 20, 61)], 8))]
    got = S.run_host(exe, d, ["D %d %s" % (parts, " ".join(map(str, own))) for parts, own in cases])
    for (parts, own), line in zip(cases, got):
        left, right = line.split("|")
        part = _lists(left)
        where = [tuple(int(x) for x in item.split(".")) for item in right.split()]
        assert [p for p, _ in part] == list(range(parts))
        assert [items for _, items in part] == [[i for i, o in enumerate(own) if o == p] for p in range(parts)]      # ascending, and each image once
        assert sorted(i for _, items in part for i in items) == list(range(len(own)))
        assert len(where) == len(own)
        for i, (p, k) in enumerate(where):
            assert p == own[i] and part[p][1][k] == i                            # (part, index) addresses the image back


def test_groups_by_chosen_strength(harness):
    exe, d = harness
    rng = np.random.default_rng(7)
    cases = [[], [19] * 6, [255, 0, 19, 0, 255], [int(v) for v in rng.integers(0, 256, 300)], [int(v) for v in rng.integers(0, 3, 40)]]
    got = S.run_host(exe, d, ["G " + " ".join(map(str, s)) for s in cases])
    for s, line in zip(cases, got):
        groups = _lists(line)
        assert groups == [(v, [i for i, x in enumerate(s) if x == v]) for v in sorted(set(s))]
        assert all(items for _, items in groups) and sorted(i for _, items in groups for i in items) == list(range(len(s)))
    assert got[0] == "" and got[2] == "0:1,3 19:2 255:0,4"


def _py_fold(rcs):
    hard = [rc for rc in rcs if rc not in (OK, ABORT)]
    return hard[0] if hard else (ABORT if ABORT in rcs else OK)


def test_fold_of_return_codes(harness):
    exe, d = harness
    codes = (OK, ABORT, HIP, BAD)
    cases = [[]] + [[c] for c in codes] + [list(p) for p in itertools.product(codes, repeat=2)] + [list(p) for p in itertools.product(codes, repeat=3)]
    got = S.run_host(exe, d, ["F " + " ".join(map(str, c)) for c in cases])
    for c, line in zip(cases, got):
        assert _ints(line) == [_py_fold(c)] * 2, c
    # spelled out: an abort before and after a hard error does not replace it, and of two hard errors the first is returned
    at = {tuple(c): _ints(line)[0] for c, line in zip(cases, got)}
    assert at[(ABORT, HIP, ABORT)] == HIP and at[(ABORT, BAD, ABORT)] == BAD
    assert at[(HIP, BAD, OK)] == HIP and at[(BAD, HIP, ABORT)] == BAD and at[(OK, BAD, HIP)] == BAD
    assert at[(OK, ABORT)] == at[(ABORT, OK)] == at[(ABORT, ABORT)] == ABORT and at[(OK, OK)] == OK and at[()] == OK

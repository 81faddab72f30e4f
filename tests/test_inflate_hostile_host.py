"""The device inflater's body (pngloss_amd/csrc/pl_inflate_core.h) on hostile streams, as a stand-alone program under -fsanitize=address,undefined
(tests/c/inflate_hostile_main.cpp), stream by stream against zlib's inflate(Z_FINISH).  Every call gets fresh heap blocks of exactly their size -- the
decoder's shared memory, the compressed bytes, the output --, so that a read behind the stream or a write behind the image is a report.  The program is
built twice: at the shipped 4 KB input stage and with -DPLI_IN=1024u, which puts stage boundaries into streams of a few KB.

The contract: where zlib ends with Z_STREAM_END after exactly `expect` bytes the decoder returns 0 and the same bytes; everywhere else it returns
non-zero.  No exceptions: there is no class of stream zlib accepts and the decoder refuses (the trailer beyond the input stage was the last one)."""
import collections
import time

import pytest

from tests import util_inflate as Z

CODES = {1: "PLI_E_HEADER", 2: "PLI_E_BLOCK", 3: "PLI_E_CODES", 4: "PLI_E_SYMBOL", 5: "PLI_E_DIST", 6: "PLI_E_SIZE", 7: "PLI_E_ADLER", 8: "PLI_E_INPUT"}
STAGES = {"stage_4096": (), "stage_1024": ("-DPLI_IN=1024u",)}
N_COMPRESSED, N_RANDOM = 12000, 8000


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_hostile")
    return {name: Z.build_hostile(d, "inflate_hostile_" + name, defs) for name, defs in STAGES.items()}


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus()


@pytest.fixture(scope="module")
def campaign():
    return Z.campaign_compressed(20261, N_COMPRESSED), Z.campaign_random_blocks(20262, N_RANDOM)


def _rows(programs, tmp_path_factory, cases, tag):
    """stage -> (the program's rows for `cases`, seconds)"""
    out = {}
    for stage, exe in programs.items():
        t0 = time.time()
        out[stage] = (Z.run_hostile(exe, tmp_path_factory.mktemp(tag + "_" + stage), cases), time.time() - t0)
    return out


@pytest.fixture(scope="module")
def corpus_rows(programs, corpus, tmp_path_factory):
    return _rows(programs, tmp_path_factory, [(z, expect) for _, z, expect, _ in corpus], "corpus")


@pytest.fixture(scope="module")
def campaign_rows(programs, campaign, tmp_path_factory):
    return _rows(programs, tmp_path_factory, [(z, expect) for z, expect, _ in campaign[0] + campaign[1]], "campaign")


def _report(title, rows, seconds):
    by = collections.Counter(r[0] for r in rows)
    print("%s: %d streams in %.2f s; zlib accepts %d, refuses %d; decoder status " % (title, len(rows), seconds, sum(r[1] for r in rows), sum(1 - r[1] for r in rows))
          + ", ".join("%s %d" % (CODES.get(k, "PLI_OK" if k == 0 else str(k)), by[k]) for k in sorted(by)))
    return by


def test_corpus_is_what_its_names_say(corpus):
    """Every hand-built stream shows what it is meant to show: zlib accepts exactly those listed as legal -- so a case cannot pass for another reason
    than the one in its name -- and the accepted ones that fit an image (expect >= 1) start with filter type none."""
    for name, z, expect, accept in corpus:
        got = Z.zlib_accepts(z, expect)
        assert (got is not None) == accept, name
        if accept and expect:
            assert got[0] == 0, name
    assert sum(c[3] for c in corpus) >= 200 and sum(not c[3] for c in corpus) >= 200, (len(corpus), sum(c[3] for c in corpus))


@pytest.mark.parametrize("stage", list(STAGES))
def test_hand_built_corpus_against_zlib(corpus, corpus_rows, stage):
    """One rule of the decoder broken per stream, by the smallest amount (tests/util_inflate.py: corpus()).  Measured: 789 streams (323 that zlib accepts),
    0.13 s for the program at the 4 KB stage, 0.17 s at the 1 KB stage; building the two sanitized programs takes 11 s."""
    rows, seconds = corpus_rows[stage]
    _report("corpus, " + stage, rows, seconds)
    for (name, z, expect, accept), (status, zaccepts, verdict) in zip(corpus, rows):
        assert zaccepts == int(accept), name                       # (the program's zlib and Python's agree)
        assert verdict == "ok" and (status == 0) == accept, (name, status, verdict)


@pytest.mark.parametrize("stage", list(STAGES))
def test_seeded_campaign_against_zlib(campaign, campaign_rows, stage):
    """12 000 compressed payloads (four kinds, zlib levels 0 / 1 / 6 / 9, five strategies, window bits 9..15) under eight mutations, and 8 000 streams of
    random bytes forced to a final fixed or dynamic block.  Seeds are constants.  So that it cannot pass vacuously, zlib alone must accept and refuse
    at least 15 % of the first generator's cases each.  Measured: 20 000 cases (84 MB of streams) in 10.4 s for the program at the 4 KB stage and 10.8 s at the
    1 KB stage, the generators 5 s; zlib accepts 3028 and refuses 8972 of the first generator's cases, 155 and 7845 of the second's."""
    first, second = campaign
    cases = first + second
    rows, seconds = campaign_rows[stage]
    _report("campaign, " + stage, rows, seconds)
    acc1, acc2 = sum(r[1] for r in rows[:len(first)]), sum(r[1] for r in rows[len(first):])
    print("first generator: zlib accepts %d, refuses %d; second: accepts %d, refuses %d" % (acc1, len(first) - acc1, acc2, len(second) - acc2))
    per = collections.Counter((Z.MUTATIONS + ("random block",))[m] for (_, _, m), r in zip(cases, rows) if r[1])
    print("accepted by zlib per mutation:", dict(per))
    assert acc1 >= 0.15 * len(first) and len(first) - acc1 >= 0.15 * len(first)
    assert acc2 >= 20                                               # accepted blocks of random bits occur
    wrong = [(i, cases[i][2], len(cases[i][0]), cases[i][1], r) for i, r in enumerate(rows) if r[2] != "ok"]
    assert not wrong, wrong[:10]


def test_every_error_code_occurs(corpus_rows, campaign_rows):
    """Over corpus and campaign every PLI_E_* code 1..8 occurs at least once, in either program."""
    for stage in STAGES:
        seen = collections.Counter(r[0] for r in corpus_rows[stage][0] + campaign_rows[stage][0])
        print(stage, {CODES.get(k, "PLI_OK"): v for k, v in sorted(seen.items())})
        assert all(seen[k] > 0 for k in CODES), (stage, dict(seen))

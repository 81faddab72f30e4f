"""The per-image result record (pngloss_amd/csrc/pl_result.h) on the CPU through tests/c/result_host.cpp: every engine's slots are disjoint and inside
the record, and the one decoder gives the pngloss_hip_result and engine_info that finish() and pngloss_hip_last_engine_info gave before it existed
(the word numbers below are written out as they stood).  The engine comes from the batch plan, not from the record: a workgroup-engine record whose
word 20 -- wave 4's light pixels -- happens to hold 3 or 4 still decodes as the workgroup engine."""
import numpy as np
import pytest

from tests import util as U

WG, SEG, ROWS = 0, 3, 4          # PLR_ENGINE_*, as lib.py's engine_info names them


def record(words=None):
    """a hand-made record: word k holds 1000 + k, so that every decoded value says where it came from; `words` {k: value} on top"""
    r = np.arange(1000, 1064, dtype=np.int32)
    for k, v in (words or {}).items():
        r[k] = v
    return r


def decode(r, engine):
    res = np.zeros(5, np.uint32)
    info = np.full(8, -7, np.int32)
    U.result_host_lib().result_host_decode(r.ctypes.data, engine, res.ctypes.data, info.ctypes.data)
    return [int(x) for x in res], [int(x) for x in info]


def test_record_is_64_words():
    assert U.result_host_lib().result_host_words() == 64


@pytest.mark.parametrize("engine", [WG, SEG, ROWS])
def test_layout_of_every_engine_is_disjoint_and_inside_the_record(engine):
    ranges = np.zeros(2 * 64, np.int32)
    k = U.result_host_lib().result_host_layout(engine, ranges.ctypes.data)
    assert k >= 7
    used = np.zeros(64, np.int32)
    for base, count in ranges[:2 * k].reshape(k, 2):
        assert count >= 1 and base >= 0 and base + count <= 64, (base, count)
        used[base:base + count] += 1
    assert used.max() == 1, np.nonzero(used > 1)
    assert list(used[:5]) == [1] * 5                  # status, bpp, unique symbols, retried rows, repaired pixels


# (engine, word 20 as that engine's kernels leave it, engine_info without the context's words 6 and 7)
CASES = [
    (SEG, 3, [3, 1005, 1004, 1006, 1007, 1017, 0, 0]),    # attempts, epochs, serial rows, none dropped, walked segments
    (WG, 1020, [0, 1005, 1004, 1021, 0, 0, 0, 0]),        # band-leader rows, pixels redone exactly, rows on the round-1 chains
    (ROWS, 4, [4, 1005, 0, 0, 0, 0, 0, 0]),               # rows
]


@pytest.mark.parametrize("engine,w20,info", CASES)
def test_decoder_gives_the_result_and_engine_info_of_each_engine(engine, w20, info):
    res, got = decode(record({20: w20}), engine)
    assert res == [1000, 1001, 1002, 1003, 1004]
    assert got == info


@pytest.mark.parametrize("light4", [3, 4])
def test_workgroup_record_whose_wave4_light_pixels_look_like_an_engine_id(light4):
    """word 20 of a workgroup-engine record is the light-pixel count of chain wave 4; read as the engine id, a count of 3 or 4 reported the segment
    or the row-statistics engine with the wrong words"""
    res, got = decode(record({20: light4}), WG)
    assert res == [1000, 1001, 1002, 1003, 1004]
    assert got == [0, 1005, 1004, 1021, 0, 0, 0, 0]


def test_abort_status_passes_through():
    res, got = decode(record({0: 65}), SEG)
    assert res[0] == 65 and got[0] == SEG

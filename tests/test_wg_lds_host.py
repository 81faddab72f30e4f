"""The shared memory of the workgroup engine (pngloss_amd/csrc/pl_wg_lds.h: one table of regions -- a fixed part and a union with three views -- from which
pl_engine.hip takes every offset and its launch's LDS bytes) on the CPU through tests/c/wg_lds_host.cpp, which lists every slot of every region.

The invariants a GPU run would only show as a corrupted neighbour or a fault: every region starts on a multiple of its alignment, the regions of the fixed part
and of each view follow one another without overlap, every view ends inside the union, every chain's records and ring stay inside the slots it takes.  And the
PINNED VALUES: every offset and byte count equals what the kernel's PL_SM_* macros gave before the table existed (literals below, computed from that code with a
host compile) -- LDS bytes decide how many workgroups share a CU, so none of them may move."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import util as U

FIXED, ROUND1, LEAD, COMMIT = range(4)
REGIONS = ["tbl", "Hc", "split_lut", "split_lut2", "costs", "pacc", "flags", "rec", "ltab", "lbs", "lwork", "lrec", "lout", "tterms"]


def constants():
    out = np.zeros(12, np.int64)
    U.wg_lds_host_lib().wg_lds_host_constants(out.ctypes.data)
    return dict(zip(["NFILT", "NSYM", "TBL_N", "TBL_DUMMY", "CHUNK", "LT_N", "LCHUNK", "LREC_N", "LRING_N", "LREC_BYTES", "LOUT_BYTES", "ALIGN_SLACK"], (int(v) for v in out)))


def chain_slot(what, i):
    return int(U.wg_lds_host_lib().wg_lds_host_chain_slot(["round1_slot", "round1_slots", "lead_table", "lead_rec_slots"].index(what), i))


def slots(layout, name):
    return [e for e in layout["entries"] if e["name"] == name]


def problems(layout):
    """every way the listing is unsound: what the header's static_assert refuses, found again from the offsets alone"""
    out = []
    entries = layout["entries"]
    union_end = layout["union_off"] + layout["union_bytes"]
    for e in entries:
        if e["align"] <= 0 or e["offset"] % e["align"]:
            out.append(("alignment", e["name"], e["slot"], e["offset"], e["align"]))
        if e["bytes"] <= 0:
            out.append(("empty", e["name"]))
    if [e["view"] for e in entries] != sorted(e["view"] for e in entries):
        out.append(("views out of carve order",))
    for view in (FIXED, ROUND1, LEAD, COMMIT):
        at = 0 if view == FIXED else layout["union_off"]
        for e in (e for e in entries if e["view"] == view):
            if e["offset"] < at:
                out.append(("overlap or out of order", e["name"], e["slot"], e["offset"], at))
            at = max(at, e["offset"] + e["bytes"])
        if view == FIXED and at != layout["union_off"]:
            out.append(("the union does not start where the fixed part ends", at, layout["union_off"]))
        if view != FIXED and at > union_end:
            out.append(("view leaves the union", view, at, union_end))
    if layout["launch_bytes"] != constants()["ALIGN_SLACK"] + union_end:
        out.append(("launch bytes", layout["launch_bytes"]))
    return out


def test_the_table_lists_the_regions_the_kernel_carves():
    lay = U.wg_lds_layout()
    k = constants()
    assert lay["regions"] == len(REGIONS) and [e["name"] for e in lay["entries"] if e["slot"] == 0] == REGIONS
    count = {name: len(slots(lay, name)) for name in REGIONS}
    assert count == dict(tbl=k["NFILT"], Hc=1, split_lut=1, split_lut2=1, costs=1, pacc=k["NFILT"], flags=1, rec=6,
                         ltab=k["NFILT"] + 1, lbs=k["NFILT"], lwork=k["NFILT"], lrec=k["NFILT"] + 1, lout=k["NFILT"], tterms=1)
    view = {e["name"]: e["view"] for e in lay["entries"]}
    assert [view[n] for n in REGIONS] == [FIXED] * 7 + [ROUND1] + [LEAD] * 5 + [COMMIT]


def test_the_layout_is_sound():
    lay = U.wg_lds_layout()
    assert lay["sound"] and problems(lay) == []
    k = constants()
    # the alignments the code relies on: 4 KB for the histogram tables, 16 B for the uint4 records and terms, 8 B for the 64-bit atomic add into pacc
    want = dict(tbl=4096, rec=16, lrec=16, tterms=16, pacc=8, costs=8, ltab=8, lout=8)
    for e in lay["entries"]:
        assert e["align"] == want.get(e["name"], 4), e
    # the five histogram tables: 4096 bytes each, on multiples of 4096 from the aligned base, bins and dummy slots inside
    tbl = slots(lay, "tbl")
    assert [(e["offset"], e["bytes"]) for e in tbl] == [(4096 * f, 4096) for f in range(k["NFILT"])]
    assert (k["NSYM"] + k["TBL_DUMMY"]) * 8 <= 4096 == k["TBL_N"] * 8
    # filter none's second decision table lies exactly PL_LT_N * 8 bytes behind its first; every other chain has one of its own
    ltab = slots(lay, "ltab")
    assert chain_slot("lead_table", 0) == 0 and ltab[1]["offset"] - ltab[0]["offset"] == k["LT_N"] * 8 == ltab[0]["bytes"]
    assert [chain_slot("lead_table", f) for f in range(k["NFILT"])] == [0, 2, 3, 4, 5] and len(ltab) == 6


def test_every_byte_count_is_the_parents():
    """the literals: the parent's PL_SM_* macros, evaluated by a host compile before this table replaced them"""
    lay = U.wg_lds_layout()
    first = {name: slots(lay, name)[0]["offset"] for name in REGIONS}
    assert (first["tbl"], first["Hc"], first["split_lut"], first["split_lut2"], first["costs"], first["pacc"], first["flags"]) == \
        (0, 20480, 21504, 23552, 25600, 25664, 25824)
    un = lay["union_off"]
    assert un == 25888 and first["rec"] == un and first["ltab"] == un and first["tterms"] == un
    assert (first["lbs"] - un, first["lwork"] - un, first["lrec"] - un, first["lout"] - un) == (24576, 34816, 37376, 65024)
    assert {e["bytes"] for e in slots(lay, "lrec")} == {4608} and {e["bytes"] for e in slots(lay, "lout")} == {2368}
    end = {view: max(e["offset"] + e["bytes"] for e in lay["entries"] if e["view"] == view) - un for view in (ROUND1, LEAD, COMMIT)}
    assert end == {ROUND1: 12288, LEAD: 76864, COMMIT: 76864}
    assert lay["union_bytes"] == 76864 and lay["commit_px"] == 4804 == 76864 // 16
    assert lay["launch_bytes"] == 106848 == 4096 + 25888 + 76864


def test_the_named_slots_keep_their_places():
    out = np.zeros(24, np.int64)
    U.wg_lds_host_lib().wg_lds_host_named(out.ctypes.data)
    v = [int(x) for x in out]
    # the seven flag words at the parent's byte offsets: big_err, big_lead, uniq, simd_map, chains_done, post_done, rowcyc
    assert [4 * w for w in v[:7]] == [0, 4, 8, 12, 20, 24, 16] and slots(U.wg_lds_layout(), "flags")[0]["bytes"] == 64
    rescan, bumped, nrel, markx, rel, rel_max, close, work_n = v[7:15]
    assert (rescan, bumped, nrel, markx, rel, rel_max, close, work_n) == (0, 32, 41, 42, 48, 64, 112, 128)
    used = sorted([(rescan, 8), (bumped, 8), (nrel, 1), (markx, 1), (rel, rel_max), (close, 8)])
    assert all(a + n <= b for (a, n), (b, _) in zip(used, used[1:])) and used[-1][0] + used[-1][1] <= work_n      # disjoint, inside the array
    assert slots(U.wg_lds_layout(), "lwork")[0]["bytes"] == 4 * work_n
    derr, cost, hs, words = v[15:19]
    assert (derr, cost, hs, words) == (0, 2, 3, 8) and hs + constants()["NFILT"] <= words and derr % 2 == 0       # (the 64-bit add needs an even word)
    assert slots(U.wg_lds_layout(), "pacc")[0]["bytes"] == 4 * words
    cc_n, lc_n, lc_build, cc_flush, lc_flush = v[19:]
    assert (cc_n, lc_n, lc_build, cc_flush, lc_flush) == (7, 8, 4, 6, 7)


def test_every_chain_stays_inside_the_slots_it_takes():
    lay = U.wg_lds_layout()
    k = constants()
    union_end = lay["union_off"] + lay["union_bytes"]

    def limit(ss, i):                     # where slot i of a region may reach: the next chain's slot, or the end of the region
        return ss[i + 1]["offset"] if i + 1 < len(ss) else ss[-1]["offset"] + ss[-1]["bytes"]

    # band-leader chains: records PL_LREC_N pixels x 4 channels (the hand-scheduled loop runs up to 4 pixels past the chunk and fetches 2 ahead), paeth two a channel
    assert k["LREC_N"] >= k["LCHUNK"] + 4 + 2
    lrec = slots(lay, "lrec")
    for f in range(k["NFILT"]):
        take = chain_slot("lead_rec_slots", f)
        assert take == (2 if f == k["NFILT"] - 1 else 1)
        need = k["LREC_N"] * 4 * k["LREC_BYTES"] * take
        assert lrec[f]["offset"] + need <= limit(lrec, f + take - 1) <= union_end, f
    assert sum(chain_slot("lead_rec_slots", f) for f in range(k["NFILT"])) == len(lrec)
    # ... result ring: (2 + PL_LCHUNK) pixels, the chunk's last two read as eight results at index n * 4 + 0..7 with n up to PL_LCHUNK
    lout = slots(lay, "lout")
    assert k["LRING_N"] >= 2 + k["LCHUNK"] + 4
    for f in range(k["NFILT"]):
        assert lout[f]["offset"] + (k["LCHUNK"] * 4 + 7 + 1) * k["LOUT_BYTES"] <= limit(lout, f) <= union_end, f
        assert (2 + k["LCHUNK"]) * 4 * k["LOUT_BYTES"] <= lout[f]["bytes"]
    # round-1 chains: wave 0 two records a channel in two slots, waves 1..4 one slot each, every index inside the six
    rec = slots(lay, "rec")
    taken = []
    for w in range(k["NFILT"]):
        s0, ns = chain_slot("round1_slot", w), chain_slot("round1_slots", w)
        assert 0 <= s0 and s0 + ns <= len(rec) == 6, w
        assert k["CHUNK"] * 4 * 16 * (2 if w == 0 else 1) <= ns * rec[0]["bytes"], w
        taken += list(range(s0, s0 + ns))
    assert taken == list(range(6))


@pytest.mark.parametrize("region", REGIONS[:-1])
def test_a_region_grown_by_16_bytes_is_noticed(region):
    """a copy of the table, one region 16 bytes longer, placed by the same function: the pins move for every region; where an alignment the code relies on
    breaks, the header's own verdict and the checks above say so too"""
    lay = U.wg_lds_layout(REGIONS.index(region), 16, 0)
    good = U.wg_lds_layout()
    assert (lay["launch_bytes"], [e["offset"] for e in lay["entries"]]) != (good["launch_bytes"], [e["offset"] for e in good["entries"]]) or \
        [e["bytes"] for e in lay["entries"]] != [e["bytes"] for e in good["entries"]]
    if region == "tbl":                   # 4112-byte tables: the second is off its 4 KB
        assert not lay["sound"] and any(p[0] == "alignment" and p[1] == "tbl" for p in problems(lay))
    elif region == "ltab":                # filter none's second table is no longer PL_LT_N * 8 behind its first
        ltab = slots(lay, "ltab")
        assert ltab[1]["offset"] - ltab[0]["offset"] != constants()["LT_N"] * 8
    else:
        assert lay["sound"] == (problems(lay) == [])


@pytest.mark.parametrize("region,grow,align", [("Hc", 4, 0), ("flags", 0, 128), ("lwork", 4, 0), ("pacc", 4, 0)])
def test_a_broken_alignment_is_reported(region, grow, align):
    """Hc four bytes longer: pacc off its 8 and the union off its 16; flags asked onto 128; a work array one word longer: the chain records off their 16;
    pacc nine words a candidate: the second candidate's 64-bit sum off its 8"""
    lay = U.wg_lds_layout(REGIONS.index(region), grow, align)
    assert not lay["sound"]
    assert any(p[0] == "alignment" for p in problems(lay))


def test_a_view_that_leaves_the_union_is_reported():
    """the listing's own check (the placement sizes the union by its chain views, so a copy cannot produce this: the listing is edited instead)"""
    lay = U.wg_lds_layout()
    lay["entries"][-1]["bytes"] += 16     # tterms, which fills the union
    assert any(p[0] == "view leaves the union" for p in problems(lay))
    lay = U.wg_lds_layout()
    slots(lay, "lbs")[0]["bytes"] += 16
    assert any(p[0] == "overlap or out of order" for p in problems(lay))


@pytest.mark.parametrize("define", ["-DPL_TBL_N=514", "-DPL_LWORK_N=129"])
def test_the_header_refuses_an_unsound_layout_at_compile_time(define):
    """the static_asserts themselves: the harness compiled with a size that breaks an alignment must not compile, and says why"""
    src = os.path.join(U.ROOT, "tests", "c", "wg_lds_host.cpp")
    with tempfile.TemporaryDirectory(prefix="wg_lds_fault_") as d:
        good = subprocess.run(U.WG_LDS_HOST_BUILD + ["-DPL_TBL_N=512", "-DPL_LWORK_N=128", "-o", os.path.join(d, "good.so"), src], capture_output=True, text=True)
        assert good.returncode == 0, good.stderr
        bad = subprocess.run(U.WG_LDS_HOST_BUILD + [define, "-o", os.path.join(d, "bad.so"), src], capture_output=True, text=True)
        assert bad.returncode != 0 and "static assertion failed" in bad.stderr and "pl_wg_lds.h" in bad.stderr, bad.stderr

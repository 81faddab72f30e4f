"""The shared memory of the segment engine's kernel bodies (pngloss_amd/csrc/pl_seg_lds.h: one layout per body, from which the body's pointers and its launch's
LDS bytes both come) on the CPU through tests/c/seg_lds_host.cpp, which lists every region of every instantiation the library ships.

The invariants a GPU run would only show as a corrupted neighbour or a fault: every region starts on a multiple of its alignment (its element size, or the widest
access a body makes to it), the regions of a layout
follow one another without overlap and end at the layout's stated end, every overlay lies inside the regions whose place it takes, and every launch asks for at
least as many bytes as the largest body its kernel dispatches needs.  And the PINNED VALUES: the bytes of every launch equal what the hand-written sums gave
before the layouts existed (literals below, recorded from that code) -- LDS bytes decide how many workgroups share a CU, so none of them may move."""
import ctypes as C

import numpy as np
import pytest

from tests import test_seg_launch_host as TL
from tests import util as U

KINDS = {0: "own", 1: "overlay", 2: "overlay behind the row before"}


def constants():
    out = np.zeros(4, np.int64)
    U.seg_lds_host_lib().seg_lds_host_constants(out.ctypes.data)
    return dict(zip(["UNIT", "CHAIN_CAP8", "CHAIN_CAP", "UNT"], (int(v) for v in out)))


def layouts(n=0):
    """name -> (end, [region dicts in carve order]); an overlay's `first` / `last` are resolved to the rows whose place it takes (its own for kind 2: the row before's)"""
    lib = U.seg_lds_host_lib()
    out = {}
    for k in range(lib.seg_lds_host_layouts()):
        name, head = C.create_string_buffer(64), np.zeros(2, np.int64)
        assert lib.seg_lds_host_layout(k, n, name, head.ctypes.data) == 0
        regions = []
        for r in range(int(head[0])):
            rn, when, v = C.create_string_buffer(64), C.create_string_buffer(128), np.zeros(7, np.int64)
            assert lib.seg_lds_host_region(k, r, n, rn, when, v.ctypes.data) == 0
            g = dict(name=rn.value.decode(), when=when.value.decode(), offset=int(v[0]), elem=int(v[1]), count=int(v[2]), kind=int(v[3]), first=int(v[4]), last=int(v[5]), align=int(v[6]))
            g["bytes"] = g["elem"] * g["count"]
            if g["kind"] == 2:
                assert regions and regions[-1]["kind"] in (1, 2), (name.value, g["name"])
                g["first"], g["last"] = regions[-1]["first"], regions[-1]["last"]
            regions.append(g)
        assert name.value.decode() not in out
        out[name.value.decode()] = (int(head[1]), regions)
    return out


def kernels():
    lib = U.seg_lds_host_lib()
    return [lib.seg_lds_host_kernel_name(k).decode() for k in range(lib.seg_lds_host_kernels())]


def launch_bytes(kernel, n=1):
    return int(U.seg_lds_host_lib().seg_lds_host_launch_bytes(kernels().index(kernel), n))


# every instantiation pl_seg.hip ships (its explicit instantiations, and what their dispatch functions call)
SHIPPED = ["enum<512>", "enum<1024>", "seeded<512>", "seeded<1024>", "small<512>", "small<1024>",
           "unit_all<UNIT>", "unit_seeds<UNIT>", "unit_small<UNIT>", "unit_all<1>", "unit_seeds<1>", "unit_small<1>",
           "first<512,false>", "first<1024,false>", "first<UNT,true>", "first<UNT,false>",
           "chain", "chain_seeded", "chain_unit", "extremes", "replay<NT>", "replay<NT_BATCH>", "post<8>", "post<16>", "commit", "ctl<TPARTS>", "ctl<TPARTS_BATCH>"]

# kernel -> the bodies it dispatches, written out from pl_seg_launch.h's seg_dispatch_* (seg_ctl_body hands the commit workgroups to seg_ctl_commit)
DISPATCHED = {
    "CTL": ["ctl<TPARTS>", "commit", "post<8>"],                                                    # seg_dispatch_ctl<SEG_TPARTS>: VGRP = SEG_VGRP_OF(TPARTS)
    "CTL_BATCH": ["ctl<TPARTS_BATCH>", "commit", "post<16>"],
    "ENUM_512": ["enum<512>", "small<512>", "first<512,false>"],                                    # seg_dispatch_enum<NT>
    "ENUM_1024": ["enum<1024>", "small<1024>", "first<1024,false>"],
    "ENUM_SEEDED_512": ["seeded<512>", "first<512,false>"],                                         # seg_dispatch_enum_seeded<NT>
    "ENUM_SEEDED_1024": ["seeded<1024>", "first<1024,false>"],
    "ENUM_UNIT": ["unit_all<UNIT>", "unit_seeds<UNIT>", "unit_small<UNIT>", "first<UNT,true>"],     # seg_dispatch_enum_unit<UNIT>: seg_first_body<SEG_UNT, (UNIT > 1)>
    "ENUM_UNIT1": ["unit_all<1>", "unit_seeds<1>", "unit_small<1>", "first<UNT,false>"],
    "GATHER_SEEDED": [],                                                                            # seg_dispatch_gather: no shared memory
    "CHAIN": ["chain", "extremes"],                                                                 # seg_dispatch_chain<SEEDED, CT, UNITS>
    "CHAIN_SEEDED": ["chain_seeded", "extremes"],
    "CHAIN_UNIT": ["chain_unit", "extremes"],
    "REPLAY": ["replay<NT>"],                                                                       # seg_dispatch_replay<RNT>
    "REPLAY_BATCH": ["replay<NT_BATCH>"],
}

# the overlays: layout -> {overlay: (first, last) region of its place}
OVERLAYS = {
    "unit": {"ht": "work", "dense": "work", "uniqr": "work", "keys": "work", "px1_seeds": "work", "mapl": "work", "px": "work", "pool2": "work"},
    "replay": {"rm": "tw", "red": "tw", "h0s": "tw"},
    "post": {"cumx": "pcw"},
    "ctl": {"spec": "stage", "ctlc": "stage", "accc": "stage", "decision": "stage", "verdict": "stage", "ecost": "stage", "failmask": "stage",
            "K": ("scratch", "basen"), "walk_state": "scratch"},                # seg_build_tables' 256 64-bit keys take scratch AND basen
}


def chain_ns():
    k = constants()
    return [1, 2, 60, 128, k["CHAIN_CAP8"] - 1, k["CHAIN_CAP8"], k["CHAIN_CAP"] + 1, 32768]


# the parent's values (SEG_SM_CHAIN(n) / SEG_SM_CHAIN_X(n) as the hand-written sums gave them), n in the order of chain_ns()
PARENT_CHAIN = [38600, 39112, 68808, 103624, 152264, 152776, 152776, 152776]
PARENT_CHAIN_X = [25536, 26048, 55744, 90560, 139200, 139712, 139712, 139712]
# ... and of the other launches: SEG_SM_CTLVAL_V(8) / (16), SEG_SM_ENUM_NT(512) / (1024), SEG_SM_ENUM_SEEDED(512) / (1024), SEG_SM_ENUM_UNIT (both kernels), SEG_SM_REPLAY
PARENT = {"CTL": 36944, "CTL_BATCH": 50992, "ENUM_512": 37568, "ENUM_1024": 40640, "ENUM_SEEDED_512": 35616, "ENUM_SEEDED_1024": 37664,
          "ENUM_UNIT": 35776, "ENUM_UNIT1": 35776, "GATHER_SEEDED": 0, "REPLAY": 49740, "REPLAY_BATCH": 49740}


def all_cases():
    """(n, name, end, regions) of every layout, the chain's at every n of chain_ns()"""
    for n in [0] + chain_ns():
        for name, (end, regions) in layouts(n).items():
            if n == 0 or name.startswith("chain"):
                yield n, name, end, regions


def test_every_shipped_instantiation_has_its_layout_listed():
    assert list(layouts()) == SHIPPED
    assert sorted(DISPATCHED) == sorted(kernels()) and sorted(set(sum(DISPATCHED.values(), []))) == sorted(SHIPPED)
    assert constants()["UNIT"] > 1                   # (seg_k_enum_unit<SEG_UNIT> and <1> are two kernels)


# the regions a body accesses with something wider than their element, written out from the bodies: layout -> {region: bytes}
WIDER = {
    "chain": {"T": 16},                              # seg_chain_body's gather: *(SegVec16 *)(T + (k << sh) + part * 8) = eight 16-bit entries
    "replay": {"red": 8},                            # PLS_ATOMIC_ADD64 on red[SEG_RR_DERR], red[SEG_RR_LB]
    "commit": {"ctlc": 8, "accc": 8},                # read as SegCtl / SegAcc (uint64_t cost[], derr[], none_lb)
    "ctl": {"ctlc": 8, "accc": 8},                   # (seg_build_tables' keys K are 64-bit elements: 8 by their type)
}


def test_every_region_starts_on_a_multiple_of_its_alignment():
    """its element size (SegPix: 8), or the widest access a body makes to it where that is wider (SegVec16: 16)"""
    seen, wider = set(), {}
    for n, name, end, regions in all_cases():
        for g in regions:
            assert g["align"] in (1, 2, 4, 8, 16) and g["offset"] % g["align"] == 0, (name, n, g)
            assert g["align"] >= g["elem"] or g["elem"] not in (1, 2, 4, 8, 16), (name, g)      # (SegState, 12 bytes of ints, states 4)
            seen.add(g["align"])
            if g["align"] != g["elem"] and g["align"] > 4:
                wider.setdefault(name.split("<")[0].split("_")[0], {})[g["name"]] = g["align"]
        assert end % 4 == 0, (name, n, end)
    assert 8 in seen and 16 in seen
    assert wider == WIDER


def test_a_layouts_own_regions_follow_one_another_and_end_at_its_end():
    for n, name, end, regions in all_cases():
        at = 0
        for g in regions:
            if g["kind"] == 0:
                assert g["offset"] == at, (name, n, g["name"], g["offset"], at)          # ascending, no overlap -- and no hole either
                at += g["bytes"]
        assert at == end, (name, n, at, end)
        assert len({g["name"] for g in regions}) == len(regions), name


def test_every_overlay_lies_inside_the_regions_whose_place_it_takes():
    seen = {}
    for n, name, end, regions in all_cases():
        prev = None
        for g in regions:
            if g["kind"] == 0:
                prev = None
                continue
            assert KINDS[g["kind"]] and 0 <= g["first"] <= g["last"] < len(regions), (name, g)
            first, last = regions[g["first"]], regions[g["last"]]
            assert first["kind"] == 0 and last["kind"] == 0, (name, g["name"])
            assert first["offset"] <= g["offset"] and g["offset"] + g["bytes"] <= last["offset"] + last["bytes"], (name, n, g, first, last)
            if g["kind"] == 1:
                assert g["offset"] == first["offset"] and g["when"], (name, g)           # it starts where its place starts, and says when it is valid
            else:
                assert g["offset"] == prev["offset"] + prev["bytes"], (name, g, prev)    # ... the next one behind it
            prev = g
            seen.setdefault(name.split("<")[0].split("_")[0], {})[g["name"]] = first["name"] if g["first"] == g["last"] else (first["name"], last["name"])
    assert seen == OVERLAYS
    # the unit enumeration's place is exactly as large as the largest of its three uses -- in every instantiation the second phase's records
    for name, (end, regions) in layouts().items():
        if name.startswith("unit"):
            by = {g["name"]: g for g in regions}
            assert by["work"]["bytes"] == by["pool2"]["offset"] + by["pool2"]["bytes"] - by["work"]["offset"] >= by["mapl"]["offset"] + by["mapl"]["bytes"] - by["work"]["offset"], name


def test_every_launch_asks_for_at_least_what_every_body_it_dispatches_needs():
    for kernel, bodies in DISPATCHED.items():
        for n in chain_ns() if kernel.startswith("CHAIN") else [1]:
            have = launch_bytes(kernel, n)
            ends = layouts(n)
            for body in bodies:
                assert have >= ends[body][0], (kernel, n, body, have, ends[body][0])
            if not bodies:
                assert have == 0


def test_the_bytes_of_every_launch_are_the_parents():
    for kernel, want in PARENT.items():
        assert launch_bytes(kernel) == want, kernel
    for n, want, want_x in zip(chain_ns(), PARENT_CHAIN, PARENT_CHAIN_X):
        assert launch_bytes("CHAIN_SEEDED", n) == want, n
        assert launch_bytes("CHAIN", n) == want_x and launch_bytes("CHAIN_UNIT", n) == want_x, n          # (CHAIN_UNIT: n units)
    # the names tests/test_seg_launch_host.py reads through its own harness are the same numbers
    k = TL.consts()
    assert (k.SM_CTLVAL, k.SM_CTLVAL_BATCH, k.SM_ENUM_512, k.SM_ENUM_1024, k.SM_ENUM_SEEDED_512, k.SM_ENUM_SEEDED_1024, k.SM_ENUM_UNIT, k.SM_REPLAY) == \
        tuple(PARENT[q] for q in ["CTL", "CTL_BATCH", "ENUM_512", "ENUM_1024", "ENUM_SEEDED_512", "ENUM_SEEDED_1024", "ENUM_UNIT", "REPLAY"])
    for n, want, want_x in zip(chain_ns(), PARENT_CHAIN, PARENT_CHAIN_X):
        assert (TL.sm_chain(n, 0), TL.sm_chain(n, 1)) == (want, want_x)


@pytest.mark.parametrize("kernel,limit", [("ENUM_1024", 65536), ("ENUM_SEEDED_1024", 65536), ("ENUM_UNIT", 65536), ("REPLAY", 65536), ("CHAIN_SEEDED", 160 * 1024), ("CTL_BATCH", 160 * 1024)])
def test_launches_stay_inside_what_they_are_launched_with(kernel, limit):
    """without an LDS opt-in: 64 KB; with one: the CU's 160 KB"""
    assert max(launch_bytes(kernel, n) for n in chain_ns()) <= limit

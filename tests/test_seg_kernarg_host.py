"""The head of the segment engine's kernels in the COMPILED code (no GPU): pl_seg.hip's device code as assembly, built by the Makefile's own rule with
the flags of its object (pngloss_amd/csrc/Makefile: pl_seg.s), read with tools/seg_heads.py.  Every kernel of a row attempt takes its explicit
arguments in scalar registers at wave launch -- the preload covers all their dwords --, lists no hidden argument (gridDim and its like would be a
scalar load of their own from the kernel-argument segment), and its kernel-argument segment is exactly the explicit arguments.  The replay kernels
request the record's fields and the whole view in one burst in front of their first branch."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from tests import util as U

HIPCC = "/opt/rocm/bin/hipcc"

# kernel (as it appears in the mangled name) -> bytes of its explicit arguments: two pointers, `par`, and what pl_seg_launch.h: SegLaunch says stands behind them
ATTEMPT_KERNELS = {
    "seg_k_ctlILi4EE": 28, "seg_k_ctlILi1EE": 28,                        # nctl, max_ngrp
    "seg_k_enumILi512EE": 28, "seg_k_enumILi1024EE": 28,                 # max_nseg, grid_x
    "seg_k_enum_seededILi512EE": 24, "seg_k_enum_seededILi1024EE": 24,   # max_nseg
    "seg_k_enum_unitILi3EE": 32, "seg_k_enum_unitILi1EE": 32,            # perb, pers, seeds
    "seg_k_gather_seeded": 24,                                           # nblk
    "seg_k_chainILb0ELi1024ELb0EE": 20, "seg_k_chainILb1ELi1024ELb0EE": 20, "seg_k_chainILb0ELi256ELb1EE": 20,
    "seg_k_replayILi1024EE": 24, "seg_k_replayILi512EE": 24,             # max_ngrp
}


def _seg_heads():
    spec = importlib.util.spec_from_file_location("seg_heads", os.path.join(U.ROOT, "tools", "seg_heads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def seg_asm(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to compile pl_seg.hip to assembly")
    out = tmp_path_factory.mktemp("seg_asm")
    r = subprocess.run(["make", "-C", os.path.join(U.ROOT, "pngloss_amd", "csrc"), "OBJDIR=%s" % out, "%s/pl_seg.s" % out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-amdgpu-kernarg-preload-count" in r.stdout            # the Makefile's flags for this file, not a copy of them
    return (out / "pl_seg.s").read_text()


def _find(table, key):
    names = [n for n in table if key in n]
    assert len(names) == 1, (key, names)
    return table[names[0]]


def test_every_attempt_kernel_is_listed(seg_asm):
    H = _seg_heads()
    names = [n for n in H.metadata(seg_asm) if "seg_k_" in n and "seg_k_resolve" not in n]
    assert len(names) == len(ATTEMPT_KERNELS)
    for n in names:
        assert sum(1 for key in ATTEMPT_KERNELS if key in n) == 1, n


@pytest.mark.parametrize("key", sorted(ATTEMPT_KERNELS))
def test_arguments_arrive_in_registers_and_none_is_hidden(seg_asm, key):
    H = _seg_heads()
    meta, desc = _find(H.metadata(seg_asm), key), _find(H.descriptors(seg_asm), key)
    explicit = ATTEMPT_KERNELS[key]
    kinds = [a[0] for a in meta["args"]]
    assert not [k for k in kinds if k.startswith("hidden")], kinds
    assert sum(1 for k in kinds if k == "global_buffer") == 2 and all(k in ("global_buffer", "by_value") for k in kinds), kinds
    assert max(off + size for _, off, size in meta["args"]) == explicit
    assert meta["kernarg_segment_size"] == explicit
    assert int(desc[".amdhsa_user_sgpr_kernarg_preload_length"]) * 4 >= explicit
    assert int(desc[".amdhsa_user_sgpr_kernarg_preload_offset"]) == 0


@pytest.mark.parametrize("key", ["seg_k_replayILi1024EE", "seg_k_replayILi512EE"])
def test_replay_requests_record_and_view_in_one_burst(seg_asm, key):
    """the replay kernels: between entry and the first vector memory instruction the code waits for scalar loads twice -- in the prologue that loads the
    arguments where the firmware does not preload them (skipped where it does), and for the record's fields with all of the view, requested together"""
    H = _seg_heads()
    listing, loads, waits = H.head(_find(H.kernels(seg_asm), key))
    assert loads >= 8 and waits == 2, (loads, waits, "\n".join(listing))
    first_branch = next(i for i, l in enumerate(listing) if "s_cbranch" in l)
    view_and_mask = [i for i, l in enumerate(listing) if "s_load_" in l and any(off in l for off in ("0x120", "0x130", "0x138", "0x158", "0x1e0"))]
    assert len(view_and_mask) >= 4 and max(view_and_mask) < first_branch, "\n".join(listing)

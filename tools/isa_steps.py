#!/usr/bin/env python3
"""isa_steps.py -- what a chain step costs in a kernel of the segment engine, from the cross-compiled assembly (no GPU needed).

Compiles pngloss_amd/csrc/pl_seg.hip to gfx950 assembly (device only) and cuts each headline kernel into basic blocks.  A block that holds chain
steps (seg_step_fast: each step reads exactly one byte of the class table, the kernels' only ds_read_u8) is listed with its steps, instructions, vector / scalar /
LDS instructions, waits for shared memory (s_waitcnt lgkmcnt), scalar compares and additions of a literal 0 (the dynamic LDS base the
linker fills in) -- per block and per step.  A rolled step loop shows as several blocks with one step between them (header, filter body, tail);
an unrolled run of N steps as one block with N steps.  Also prints every kernel's code size.
(tools/isa_rounds.py answers another question -- where a kernel waits for DEVICE memory, vmcnt rounds by source line -- and knows nothing of steps,
shared-memory waits or basic blocks; this one needs no line info.)

usage: tools/isa_steps.py [extra hipcc flags, e.g. -DSEG_K1_ONE_CHUNK=2]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pngloss_amd", "csrc", "pl_seg.hip")
KERNELS = [("seg_k_enum<512>", "seg_k_enumILi512E"), ("seg_k_ctl<4>", "seg_k_ctlILi4E"), ("seg_k_replay<1024>", "seg_k_replayILi1024E"),
           ("seg_k_chain<false,1024,false>", "seg_k_chainILb0ELi1024ELb0E")]


def blocks(body):
    """basic blocks: cut at labels and behind branches"""
    cur, out = [], []
    for l in body:
        if re.match(r"^\.LBB\d+_\d+:", l):
            if cur:
                out.append(cur)
            cur = [l]
            continue
        if not re.match(r"^\t[a-z]", l) or l.startswith("\t."):
            continue
        cur.append(l.strip().split(";")[0].strip())
        if re.match(r"^\ts_(cbranch|branch|endpgm|setpc)", l):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="isa_steps_")
    try:
        asm = os.path.join(tmp, "pl_seg.s")
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, SRC] + sys.argv[1:],
                           capture_output=True, text=True, cwd=os.path.dirname(SRC))
        if r.returncode:
            sys.exit("isa_steps: hipcc failed\n" + r.stderr[-4000:])
        src = open(asm).read().split("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for name, pat in KERNELS:
        found = [i for i, l in enumerate(src) if re.match(r"^_ZN12_GLOBAL__N_1\d+" + pat + r"\S*:", l)]
        if not found:
            sys.exit("isa_steps: kernel %s is not in the assembly" % name)
        a = found[0]
        b = [i for i, l in enumerate(src) if i > a and ".amdhsa_kernel" in l][0]
        size = re.search(r"codeLenInByte = (\d+)", "\n".join(src[a:b + 400])).group(1)
        body = src[a:b]
        ins = [l for l in body if re.match(r"^\t[a-z]", l) and not l.startswith("\t.")]
        zero = sum(1 for l in ins if re.match(r"^\tv_add(3)?_u32(_e32|_e64)? v\d+, 0, ", l))
        print("%s: codeLenInByte %s, %d instructions, %d additions of a literal 0" % (name, size, len(ins), zero))
        n = 0
        for blk in blocks(body):
            code = [l for l in blk if not l.endswith(":")]
            steps = sum(1 for l in code if re.match(r"ds_read_u8 ", l))
            if not steps:
                n += len(code)
                continue
            cnt = lambda p: sum(1 for l in code if re.match(p, l))
            label = blk[0][:-1] if blk[0].endswith(":") else "(fall-through)"
            print("  +%5d %-12s %2d steps %4d instr (%5.1f a step): valu %4d salu %3d ds %3d, lgkm waits %3d (%.1f a step), s_cmp %d, adds of 0: %d"
                  % (n, label, steps, len(code), len(code) / steps, cnt(r"v_"), cnt(r"s_(?!waitcnt|nop|cbranch|branch)"), cnt(r"ds_"),
                     cnt(r"s_waitcnt.*lgkmcnt"), cnt(r"s_waitcnt.*lgkmcnt") / steps, cnt(r"s_cmp"), cnt(r"v_add(3)?_u32(_e32|_e64)? v\d+, 0, ")))
            n += len(code)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The HEAD of the segment engine's kernels in the compiled code: from a kernel's entry to its first vector memory
instruction, with the scalar round trips (s_waitcnt that waits for lgkmcnt with scalar loads outstanding) counted.

  hipcc <the Makefile's flags for pl_seg.hip> --cuda-device-only -S pngloss_amd/csrc/pl_seg.hip -o seg.s
  python tools/seg_heads.py seg.s [kernel-name-substring ...]        (default: the three kernels of one image's attempt)

Also usable as a module (tests/test_seg_kernarg_host.py): kernels(text) -> {name: lines}, head(lines), descriptors(text), metadata(text)."""
import re
import sys

DEFAULT = ["seg_k_replayILi1024EE", "seg_k_chainILb0ELi1024ELb0EE", "seg_k_enumILi512EE"]
VMEM = re.compile(r"^\s*(global_|flat_|buffer_|scratch_)")
SLOAD = re.compile(r"^\s*s_(buffer_)?load_")
WAIT = re.compile(r"^\s*s_waitcnt\b.*lgkmcnt\((\d+)\)")


def kernels(text):
    """{mangled name: instruction lines of the function body (labels and comments-only lines dropped)}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):\s*;\s*@", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if s.strip() and not s.lstrip().startswith("."):
            cur.append(s)
        elif s.lstrip().startswith(".LBB"):
            cur.append(s)
    return out


def head(lines):
    """(the listing up to and including the first vector memory instruction, scalar loads in it, waits that had scalar loads outstanding)"""
    listing, loads, waits, pending = [], 0, 0, 0
    for s in lines:
        listing.append(s)
        if SLOAD.match(s):
            loads += 1
            pending += 1
        m = WAIT.match(s)
        if m and pending > int(m.group(1)):
            waits += 1
            pending = int(m.group(1))
        if VMEM.match(s):
            break
    return listing, loads, waits


def descriptors(text):
    """{kernel: {directive: value}} of the .amdhsa_kernel blocks"""
    out, cur = {}, None
    for line in text.splitlines():
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = out.setdefault(t.split()[1], {})
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            p = t.split()
            cur[p[0]] = p[1] if len(p) > 1 else ""
    return out


def metadata(text):
    """{kernel: {"kernarg_segment_size": n, "args": [(value_kind, offset, size), ..]}} from the amdhsa.kernels note"""
    out = {}
    m = re.search(r"^amdhsa\.kernels:\s*$(.*?)^amdhsa\.", text, re.S | re.M)
    if not m:
        return out
    for block in re.split(r"^  - \.agpr_count:", m.group(1), flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        args = []
        for a in re.split(r"^\s+- ", block.split(".args:")[1].split(".group_segment_fixed_size")[0], flags=re.M) if ".args:" in block else []:
            k = re.search(r"\.value_kind:\s+(\S+)", a)
            if k:
                args.append((k.group(1), int(re.search(r"\.offset:\s+(\d+)", a).group(1)), int(re.search(r"\.size:\s+(\d+)", a).group(1))))
        out[name] = {"kernarg_segment_size": int(re.search(r"\.kernarg_segment_size:\s+(\d+)", block).group(1)), "args": args,
                     "sgpr_count": int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)), "sgpr_spill_count": int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))}
    return out


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2:] or DEFAULT
    ks, ds, ms = kernels(text), descriptors(text), metadata(text)
    for name, lines in ks.items():
        if not any(w in name for w in want):
            continue
        listing, loads, waits = head(lines)
        d, m = ds.get(name, {}), ms.get(name, {})
        print("== %s" % name)
        print("   entry to first vector memory instruction: %d instructions, %d scalar loads, %d waits for scalar loads; kernarg preload length %s dwords; whole kernel: %s SGPRs, %s spilled"
              % (len(listing), loads, waits, d.get(".amdhsa_user_sgpr_kernarg_preload_length", "?"), m.get("sgpr_count", "?"), m.get("sgpr_spill_count", "?")))
        for s in listing:
            print(s)
        print()


if __name__ == "__main__":
    main()

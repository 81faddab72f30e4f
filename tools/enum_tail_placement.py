"""Developer tool (GPU box): where the enumeration's tail waves sit, and what sharing a SIMD costs them.

Needs a MEASUREMENT BUILD of the library (-DSEG_EXPERIMENT_TAIL_PLACEMENT=1, tools/build_variant.sh), named by PNGLOSS_HIP_LIBNAME: seg_enum_body_k then leaves
one record per workgroup (of the first 1024 of a launch, for the launches of sixteen rows) in a buffer of its own: HW_ID and XCC_ID of the wave that walks the
steps behind the dedupe, the phase in 100 MHz ticks and in shader cycles, the SIMD of every wave of the workgroup, HW_ID of wave 0, and the 100 MHz clock at the
body's head, the tail's head and its end.

usage: PNGLOSS_HIP_LIBNAME=libpngloss_hip_NAME.so python tools/enum_tail_placement.py [W [H [s [b]]]]      (4096 16 19 2: the headline's row)
Prints (a) a histogram of tail waves per (CU, SIMD), launch by launch, (b) the tail's time per step grouped by how many tail waves shared the SIMD, and (c) the
workgroups of a launch on one clock, candidate by candidate: when they start, how long their phases take, which ends last."""
import collections
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pngloss_amd as P  # noqa: E402
from pngloss_amd import lib, synth  # noqa: E402

ROWS, WGS, WORDS = 16, 1024, 12
TAIL_STEPS = 28


def fields(hw):
    """HW_ID of gfx9: WAVE_ID 3:0, SIMD_ID 5:4, PIPE_ID 7:6, CU_ID 11:8, SH_ID 12, SE_ID 15:13, TG_ID 19:16"""
    return {"slot": hw & 15, "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7, "tg": (hw >> 16) & 15}


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    s = int(sys.argv[3]) if len(sys.argv) > 3 else 19
    b = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    h = lib.hip_lib()
    fn = h.pngloss_hip_debug_tail_placement
    fn.restype, fn.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t]
    img = synth.synth_rgba(W, H, 0, 0)
    lib.optimize_with_rows(img, s, b)
    buf = np.zeros(ROWS * WGS * WORDS, np.uint32)
    assert fn(buf.ctypes.data, buf.size) == buf.size, "no records: not a measurement build?"
    rec = buf.reshape(ROWS, WGS, WORDS)
    print(f"# {W}x{H} mode 0 s={s} b={b}, library {os.environ.get('PNGLOSS_HIP_LIBNAME', 'libpngloss_hip.so')}, source_digest={P.source_digest()}")
    by_share_ticks, by_share_cyc = collections.defaultdict(list), collections.defaultdict(list)
    hist = collections.Counter()
    per_cu_hist = collections.Counter()
    wave0_simd, tail_simd, tgs, slots0, orders = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    tg_distinct = collections.Counter()
    launches = 0
    first = True
    for y in range(ROWS):
        r = rec[y][(rec[y][:, 7] >> 31) == 1]
        if not len(r):
            continue
        launches += 1
        place = collections.defaultdict(list)
        cus = collections.defaultdict(list)
        for k, w in enumerate(r):
            t, w0 = fields(int(w[0])), fields(int(w[6]))
            cu = (int(w[1]) & 15, t["se"], t["sh"], t["cu"])
            place[cu + (t["simd"],)].append(k)
            cus[cu].append((t["simd"], t["tg"], w0["slot"], w0["simd"]))
            wave0_simd[w0["simd"]] += 1
            tail_simd[t["simd"]] += 1
            tgs[t["tg"]] += 1
            slots0[w0["slot"]] += 1
            orders["".join(str((int(w[5]) >> (2 * q)) & 3) for q in range(8))] += 1
        launch_hist = collections.Counter(len(v) for v in place.values())
        for n, c in launch_hist.items():
            hist[n] += c
        for cu, v in cus.items():
            simds = collections.Counter(x[0] for x in v)
            per_cu_hist[(len(v), max(simds.values()))] += 1
            tg_distinct[(len(v), len(set(x[1] & 3 for x in v)))] += 1
        for key, ks in place.items():
            for k in ks:
                by_share_ticks[len(ks)].append(int(r[k][2]))
                by_share_cyc[len(ks)].append(int(r[k][3]))
        if first:
            first = False
            print(f"# one launch (row {y}): {len(r)} workgroups of seg_enum_body on {len(cus)} CUs; tail waves per (CU, SIMD) -> number of (CU, SIMD) pairs: " +
                  ", ".join(f"{n}: {c}" for n, c in sorted(launch_hist.items())))
    print(f"== (a) tail waves per (CU, SIMD), {launches} launches together: (CU, SIMD) pairs holding n tail waves")
    for n, c in sorted(hist.items()):
        print(f"n={n}: {c}")
    print("   per CU and launch: (tail waves on the CU, most on one SIMD) -> CUs")
    for k, c in sorted(per_cu_hist.items()):
        print(f"   {k[0]} on the CU, {k[1]} on one SIMD: {c}")
    print("   SIMD of the tail wave:", dict(sorted(tail_simd.items())), " SIMD of wave 0:", dict(sorted(wave0_simd.items())))
    print("   wave slot of wave 0:", dict(sorted(slots0.items())), " TG_ID:", dict(sorted(tgs.items())))
    print("   per CU and launch: (workgroups on the CU, distinct TG_ID mod 4 among them) -> CUs:", dict(sorted(tg_distinct.items())))
    print("   SIMD of waves 0..7 of a workgroup, the commonest orders:", orders.most_common(6))
    print(f"== (b) the tail phase ({TAIL_STEPS} steps), grouped by the tail waves that shared its (CU, SIMD) in the launch")
    for n in sorted(by_share_ticks):
        t, c = by_share_ticks[n], by_share_cyc[n]
        print(f"shared by {n}: {len(t)} tails; us median {statistics.median(t) / 100:.2f} mean {statistics.fmean(t) / 100:.2f} max {max(t) / 100:.2f}; "
              f"us a step {statistics.fmean(t) / 100 / TAIL_STEPS:.3f}; shader cycles a step median {statistics.median(c) / TAIL_STEPS:.0f} mean {statistics.fmean(c) / TAIL_STEPS:.0f}")
    allt = [x for v in by_share_ticks.values() for x in v]
    print(f"all: {len(allt)} tails, us mean {statistics.fmean(allt) / 100:.2f}, us a step {statistics.fmean(allt) / 100 / TAIL_STEPS:.3f}")
    # (c) a launch as its workgroups see it: the 100 MHz clock is one for the device, so the heads and ends of a launch's workgroups compare
    names = {1: "sub", 3: "avg", 4: "paeth", 0: "none", 2: "up"}
    by_f = collections.defaultdict(lambda: collections.defaultdict(list))
    spans, last_f, last_two = [], collections.Counter(), collections.Counter()
    for y in range(ROWS):
        r = rec[y][(rec[y][:, 7] >> 31) == 1]
        if not len(r):
            continue
        t0 = int(r[:, 8].min())
        rel = lambda a: ((a.astype(np.int64) - t0) & 0xffffffff) / 100.0          # us behind the first head of the launch
        head, th, te = rel(r[:, 8]), rel(r[:, 9]), rel(r[:, 10])
        spans.append(float(te.max()))
        k = int(te.argmax())
        last_f[names[int(r[k][7]) & 255]] += 1
        last_two[int(r[k][4]) > 64] += 1
        for q, w in enumerate(r):
            d = by_f[names[int(w[7]) & 255]]
            d["head"].append(head[q]); d["front"].append(th[q] - head[q]); d["tail"].append(te[q] - th[q]); d["end"].append(te[q]); d["two"].append(int(w[4]) > 64); d["states"].append(int(w[4]))
    print("== (c) the workgroups of a launch on one clock (us behind the launch's first workgroup head), by candidate")
    for f, d in sorted(by_f.items()):
        print(f"{f}: {len(d['head'])} workgroups; head mean {statistics.fmean(d['head']):.2f} max {max(d['head']):.2f}; load + first steps + dedupe mean {statistics.fmean(d['front']):.2f} max {max(d['front']):.2f}; "
              f"tail mean {statistics.fmean(d['tail']):.2f} max {max(d['tail']):.2f}; end mean {statistics.fmean(d['end']):.2f} max {max(d['end']):.2f}; "
              f"states mean {statistics.fmean(d['states']):.1f}, more than 64 (a second tail wave) in {sum(d['two'])}")
        one = [t for t, two in zip(d['tail'], d['two']) if not two]
        two = [t for t, tw in zip(d['tail'], d['two']) if tw]
        if two:
            print(f"   tail with one wave mean {statistics.fmean(one):.2f}, with two {statistics.fmean(two):.2f}")
    print(f"   last end of a launch: mean {statistics.fmean(spans):.2f}, min {min(spans):.2f}, max {max(spans):.2f}; the last workgroup's candidate: {dict(last_f)}; it had a second tail wave: {dict(last_two)}")


if __name__ == "__main__":
    main()

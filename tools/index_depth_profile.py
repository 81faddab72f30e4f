"""The measurements of the option "index_depth" in profiles/index_depth.txt: pngloss_hip_optimize_batch_host_zlib at strength 0 with
"indexed" on, on uniformly random 16-colour frames -- `big`: one 4096x4096 frame; `frames`: 256 frames of 1920x1080 (8 distinct ones).  Only the C
call is timed (host clock around the synchronous call, and the library's own deflate-stage time): buffers are prepared once.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/index_depth_profile.py trace big|frames CALLS
        "index_depth" at "min", one small warm-up call, then CALLS calls: the kernel trace has pl_index_pack (and pl_index_rows beside it)
  python tools/index_depth_profile.py cost big|frames ROUNDS CALLS
        ROUNDS alternating rounds of "8", "auto", "min": median call and deflate-stage time of CALLS calls each, and the bytes of all streams
  python tools/index_depth_profile.py ab big|frames CALLS
        the option never set: medians of CALLS calls.  With PNGLOSS_HIP_LIBNAME=/path/to/the/parent's/libpngloss_hip.so the same call on the parent
        commit's library (which lacks the new accessors: their prototypes are dropped first); alternate the two processes for an A/B."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pngloss_amd.lib as L
if os.environ.get("PNGLOSS_HIP_LIBNAME"):          # the parent's library has no index_depth accessors
    L.INDEX_DEPTH_PROTOTYPES.clear()
import pngloss_amd as P
from tests import util_index_depth as D


def inputs(name):
    if name == "big":
        return [D.noise(16, 4096, 4096, 21)]
    if name == "frames":
        distinct = [D.noise(16, 1920, 1080, 30 + k) for k in range(8)]
        return [distinct[k % 8] for k in range(256)]
    if name == "small":
        return [D.noise(16, 64, 64, 3)]
    raise SystemExit("input?")


class Call:
    """the zlib call on prepared buffers: only the C call is timed"""
    def __init__(self, ctx, arrays):
        self.ctx, self.n = ctx, len(arrays)
        self.outs, self.filts, self.imgs = L._host_images(arrays, True)
        self.zs, self.bufs = L._zstreams(ctx._lib, [(a.shape[1], a.shape[0]) for a in self.outs])
        self.res = L._array(L.Result, self.n)

    def __call__(self):
        t0 = time.perf_counter()
        rc = self.ctx._lib.pngloss_hip_optimize_batch_host_zlib(self.ctx._ctx, self.imgs, self.n, 0, 2, self.res, self.zs)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt, self.ctx.deflate_ms


def med(xs):
    return round(statistics.median(xs), 2)


mode, name = sys.argv[1], sys.argv[2]
ctx = P.HipContext()
ctx.set_option("indexed", "on")
if mode == "trace":
    ctx.set_option("index_depth", "min")
    Call(ctx, inputs("small"))()
    c = Call(ctx, inputs(name))
    for _ in range(int(sys.argv[3])):
        print("trace", name, c(), flush=True)
    d = ctx.index_depth(0).as_dict()
    print("record", d, flush=True)
elif mode == "cost":
    rounds, calls = int(sys.argv[3]), int(sys.argv[4])
    c = Call(ctx, inputs(name))
    for m in ("8", "auto", "min"):
        ctx.set_option("index_depth", m)
        c()                                        # warm-up of every configuration (grows the workspace)
    out = []
    for r in range(rounds):
        for m in ("8", "auto", "min"):
            ctx.set_option("index_depth", m)
            t = [c() for _ in range(calls)]
            row = dict(input=name, round=r + 1, mode=m, call_ms=med([a for a, _ in t]), deflate_ms=med([b for _, b in t]), calls=calls,
                       total_stream_bytes=int(sum(z.size for z in c.zs[:c.n])))
            print(json.dumps(row), flush=True)
elif mode == "ab":
    calls = int(sys.argv[3])
    c = Call(ctx, inputs(name))
    c(); c()
    t = [c() for _ in range(calls)]
    print(json.dumps(dict(input=name, lib=os.environ.get("PNGLOSS_HIP_LIBNAME", "this tree"), call_ms=med([a for a, _ in t]), deflate_ms=med([b for _, b in t]),
                          min_call_ms=round(min(a for a, _ in t), 2), max_call_ms=round(max(a for a, _ in t), 2), calls=calls,
                          streams=[int(z.size) for z in c.zs[:c.n]][:4])), flush=True)
ctx.close()

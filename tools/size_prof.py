"""What a size search costs: the 4096x4096 headline frame (or, with `batch`, 32 frames of 1920x1080 as one batch) through
pngloss_hip_optimize_batch_size with M = 19, bleed 2 and a budget per frame that lands strictly inside 0..19, next to what a user's own loop pays
in the same process: plain runs at strength 19 and one-probe size calls (a budget of 1 byte, which nothing meets) without and with the streams
wanted.  Prints probes, runs and the wall time of the size call with its spread.  The differences of those public calls hold more than the two
deflates (emit, moves, the measuring kernel of the report), so pl_deflate_measure against pl_deflate_images comes from the library's own clocks:
a child process runs the one-probe call with streams under PNGLOSS_HIP_DEBUG=1, where deflate_group prints its phases for both modes -- the same
scanlines, the same process, like against like.

    python tools/size_prof.py [batch] [REPEATS]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pngloss_amd as P  # noqa: E402

import re  # noqa: E402
import subprocess  # noqa: E402

args = sys.argv[1:]
phases_child = bool(args) and args[0] == "phases"
if phases_child:
    args = args[1:]
batch = bool(args) and args[0] == "batch"
if batch:
    args = args[1:]
REPEATS = int(args[0]) if args else 5
M, BLEED, NEVER = 19, 2, 1        # a budget of 1 byte is never met: one probe at M, whose result and size are kept
shapes = [(1920, 1080, 0, f) for f in range(32)] if batch else [(4096, 4096, 0, 0)]
frames = [P.synth_rgba(w, h, mode, f) for (w, h, mode, f) in shapes]
src = [torch.from_numpy(a).cuda() for a in frames]
filt = [torch.zeros(a.shape[0], dtype=torch.uint8, device="cuda") for a in frames]
ctx = P.HipContext()


def fresh():
    work = [s.clone() for s in src]
    torch.cuda.synchronize()
    return work, [(w.data_ptr(), f.data_ptr(), a.shape[1], a.shape[0]) for w, f, a in zip(work, filt, frames)]


def timed(fn):
    work, desc = fresh()
    t0 = time.perf_counter()
    out = fn(desc)
    return time.perf_counter() - t0, out


def spread(xs):
    return "median %.1f ms (min %.1f, max %.1f, n = %d)" % (1e3 * statistics.median(xs), 1e3 * min(xs), 1e3 * max(xs), len(xs))


if phases_child:
    for _ in range(REPEATS + 1):                                 # (the first repetition warms up and is dropped by the parent)
        timed(lambda d: ctx.run_size(d, [NEVER] * len(frames), M, BLEED, want_streams=True))
    ctx.close()
    sys.exit(0)

# budgets strictly inside: halfway between the streams of strengths 9 and 19, per frame (one-probe calls measure them)
size = {}
for s in (9, 19):
    _, (_, rep, _) = timed(lambda d: ctx.run_size(d, [NEVER] * len(frames), s, BLEED))
    size[s] = [r.bytes for r in rep]
budgets = [(a + b) // 2 for a, b in zip(size[9], size[19])]
print("stream of frame 0: strength 9 %d bytes, strength 19 %d bytes; budget %d, M = %d" % (size[9][0], size[19][0], budgets[0], M))

plain_s = [timed(lambda d: ctx.run(d, M, BLEED))[0] for _ in range(REPEATS)]
measure_s = [timed(lambda d: ctx.run_size(d, [NEVER] * len(frames), M, BLEED))[0] for _ in range(REPEATS)]
write_s = [timed(lambda d: ctx.run_size(d, [NEVER] * len(frames), M, BLEED, want_streams=True))[0] for _ in range(REPEATS)]
search_s, reps = [], None
for _ in range(REPEATS):
    dt, (_, reps, _) = timed(lambda d: ctx.run_size(d, budgets, M, BLEED))
    search_s.append(dt)
runs = max(r.runs for r in reps)
print("chosen strengths %s, probes %s, runs %s, reached %s" % (sorted({r.strength for r in reps}), sorted({r.probes for r in reps}), sorted({r.runs for r in reps}),
                                                          sorted({r.reached for r in reps})))
print("plain run at %d:                       %s" % (M, spread(plain_s)))
print("one probe, measured (run + emit + pl_deflate_measure): %s" % spread(measure_s))
print("one probe, measured and written (+ pl_deflate_images):   %s" % spread(write_s))
child = subprocess.run([sys.executable, os.path.abspath(__file__), "phases"] + (["batch"] if batch else []) + [str(REPEATS)], capture_output=True, text=True,
                       env=dict(os.environ, PNGLOSS_HIP_DEBUG="1"))
lines = {"measure": [], "write": []}
for ln in child.stderr.splitlines():
    mt = re.match(r"pngloss_hip deflate( \(measure only\))?: .*?: alloc ([\d.]+) ms, kernels ([\d.]+) ms, gather ([\d.]+) ms, download ([\d.]+) ms, free ([\d.]+) ms", ln)
    if mt:
        lines["measure" if mt.group(1) else "write"].append([float(x) for x in mt.groups()[1:]])
for kind, name in (("measure", "pl_deflate_measure"), ("write", "pl_deflate_images ")):
    rows = lines[kind][1:]
    if rows:
        tot = [sum(r) for r in rows]
        med = [statistics.median(c) for c in zip(*rows)]
        print("%s (library clocks): median %.1f ms (min %.1f, max %.1f, n = %d); phases alloc %.1f, kernels %.1f, gather %.1f, download %.1f, free %.1f"
              % (name, statistics.median(tot), min(tot), max(tot), len(tot), *med))
m_ms = [1e3 * (a - statistics.median(plain_s)) for a in measure_s]
w_ms = [1e3 * (b - a) for a, b in zip(measure_s, write_s)]
print("differences of public calls (not the functions alone): measured probe - plain run: median %.1f ms (min %.1f, max %.1f); written - measured probe: median %.1f ms (min %.1f, max %.1f)"
      % (statistics.median(m_ms), min(m_ms), max(m_ms), statistics.median(w_ms), min(w_ms), max(w_ms)))
print("size call:                              %s" % spread(search_s))
loop = [runs * (p + w / 1e3) for p, w in zip(plain_s, w_ms)]
print("a user's loop of %d plain runs + %d writing deflates: %s; the size call costs %.2f x that (per-repetition ratios %s)"
      % (runs, runs, spread(loop), statistics.median(search_s) / statistics.median(loop), ", ".join("%.2f" % (a / b) for a, b in zip(search_s, loop))))
ctx.close()

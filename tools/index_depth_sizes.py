"""The file sizes in profiles/index_depth.txt: the tool with --colors 2 / 4 / 16, with and without --dither, over the eleven suite images
(tests/golden/suite_png.npz) without --index-depth ("8") and with it at auto and min.  One line of totals per configuration -- with how often the
8-bit file is smaller than the packed one --, then per file: colours, dither, image, bytes at "8", "auto", "min".
usage: python tools/index_depth_sizes.py [rows.json]"""
import json, os, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import util as U
CLI = os.path.join(U.ROOT, "pngloss_amd", "cli", "pngloss")
g = U.load_npz("suite_png.npz")
names = sorted(g.files)
d = tempfile.mkdtemp(prefix="sizes_")
for n in names:
    open(os.path.join(d, n + ".png"), "wb").write(g[n].tobytes())
rows = []
for colors in (2, 4, 16):
    for dither in (False, True):
        sizes = {}
        for mode in ("8", "auto", "min"):
            args = [CLI, "-f", "--ext", f"-{mode}.png", "--colors", str(colors)] + (["--dither"] if dither else []) + (["--index-depth", mode] if mode != "8" else [])
            r = subprocess.run(args + [os.path.join(d, n + ".png") for n in names], capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                print("FAILED", args, r.returncode, r.stderr[-500:], flush=True)
                sys.exit(r.returncode if r.returncode > 0 else 1)
            sizes[mode] = {n: os.path.getsize(os.path.join(d, f"{n}-{mode}.png")) for n in names}
        for n in names:
            rows.append(dict(colors=colors, dither=dither, image=n, **{m: sizes[m][n] for m in sizes}))
        tot = {m: sum(sizes[m].values()) for m in sizes}
        beats = sum(1 for n in names if sizes["8"][n] < sizes["min"][n])
        auto_is_best = all(sizes["auto"][n] <= min(sizes["8"][n], sizes["min"][n]) for n in names)
        print(json.dumps(dict(colors=colors, dither=dither, total=tot, eight_bit_beats_packed=beats, of=len(names), auto_never_larger=auto_is_best)), flush=True)
if len(sys.argv) > 1:
    json.dump(rows, open(sys.argv[1], "w"), indent=0)
for r in rows:
    print(r["colors"], int(r["dither"]), r["image"], r["8"], r["auto"], r["min"])

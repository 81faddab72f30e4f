"""Writes tests/golden/size_target_table.json: what the size search must find for the fixed cases, from the CPU alone.

Each probe is U.run_port -> U.png_scanlines_reference -> U.deflate_host -> length (tests/util_size.py: oracle_size); the budgets come from that same
chain, and the rule is the Python restatement S.py_search.  The generator ASSERTS that the table holds every class of outcome -- unreachable at M,
met only at M, met at an interior strength, met at strength 0 -- and that the large image has two deflate blocks; it also lists every place where
the size is not monotone in the strength (DESIGN.md section 10c names them).

    python tests/golden/make_size_target_table.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import util_size as S  # noqa: E402
from tests import util_target as T  # noqa: E402

#: (width, height, synth mode), M
SHAPES = [((64, 16, 0), 19), ((130, 6, 3), 19), ((7, 5, 1), 19), ((300, 300, 0), 19), ((33, 16, 2), 40)]


def classify(chosen, reached, m):
    if not reached:
        return "unreachable"
    return "at_0" if chosen == 0 else "only_at_M" if chosen == m else "interior"


def main():
    cases, non_monotone, sizes_out = [], [], {}
    for shape, m in SHAPES:
        w, h, mode = shape
        sizes = [S.oracle_size(w, h, mode, s)[0] for s in range(m + 1)]
        sizes_out["%dx%d_mode%d" % shape] = sizes
        for s in range(m):
            if sizes[s + 1] > sizes[s]:
                non_monotone.append(dict(shape=list(shape), strength=s + 1, bytes=sizes[s + 1], below=sizes[s]))
        budgets = sorted({sizes[m] - 1, sizes[m], sizes[0], sizes[0] + 100, sizes[m // 2], sizes[m // 3], (sizes[0] + sizes[m]) // 2, min(sizes), 2 ** 63})
        for budget in budgets:
            if budget < 1:
                continue
            chosen, reached, seq, kept = S.oracle_search(shape, m, budget)
            cases.append(dict(shape=list(shape), M=m, budget=budget, chosen=chosen, reached=reached, probes=seq, bytes=kept,
                              color_type=S.oracle_size(w, h, mode, chosen)[1], outcome=classify(chosen, reached, m)))
    seen = {c["outcome"] for c in cases}
    assert seen == {"unreachable", "only_at_M", "interior", "at_0"}, seen
    for shape, m in SHAPES:
        assert {c["outcome"] for c in cases if c["shape"] == list(shape)} >= {"unreachable", "at_0"}, shape
    big = T.oracle_probe(300, 300, 0, 19)
    assert len(S.scanline_bytes(big[1], big[2])[1]) > 262144         # two deflate blocks
    assert all(len(c["probes"]) <= S.py_probe_bound(c["M"]) for c in cases)
    with open(S.TABLE, "w") as fh:
        json.dump(dict(bleed=S.BLEED, cases=cases, sizes=sizes_out, non_monotone=non_monotone), fh, indent=1)
        fh.write("\n")
    print("%d cases, outcomes %s, %d non-monotone steps" % (len(cases), sorted(seen), len(non_monotone)))
    for x in non_monotone:
        print("  not monotone:", x)


if __name__ == "__main__":
    main()

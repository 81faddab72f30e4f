"""The pinned table of the size search (tests/golden/size_target_table.json, written by tests/golden/make_size_target_table.py) against the CPU chain
it was made from -- U.run_port -> U.png_scanlines_reference -> U.deflate_host -> length -- and the rule restated in Python (tests/util_size.py).
No code under test runs here; tests/test_gpu_size.py compares the library with this table."""
from tests import util_size as S

OUTCOMES = {"unreachable", "only_at_M", "interior", "at_0"}


def test_table_holds_every_outcome_and_respects_the_bound():
    t = S.load_table()
    assert t["bleed"] == S.BLEED
    assert {c["outcome"] for c in t["cases"]} == OUTCOMES
    for c in t["cases"]:
        assert len(c["probes"]) <= S.py_probe_bound(c["M"]) and c["probes"][0] == c["M"]
        assert c["reached"] == int(c["bytes"] <= c["budget"])
        assert (c["outcome"] == "unreachable") == (not c["reached"]) and (c["chosen"] == c["M"] or c["reached"])
    assert any(c["shape"] == [300, 300, 0] and c["outcome"] == "interior" for c in t["cases"])      # the two-block image searches, too
    assert t["non_monotone"]                                     # the size is not monotone in the strength: the result is defined by the procedure


def test_a_subset_recomputed_on_the_cpu():
    t = S.load_table()
    small = [c for c in t["cases"] if c["shape"][0] * c["shape"][1] < 5000]
    big = [c for c in t["cases"] if c["shape"] == [300, 300, 0] and c["outcome"] in ("interior", "unreachable")][:2]
    assert len(small) >= 20 and len(big) == 2
    for c in small + big:
        chosen, reached, seq, kept = S.oracle_search(tuple(c["shape"]), c["M"], c["budget"])
        assert (chosen, reached, seq, kept) == (c["chosen"], c["reached"], c["probes"], c["bytes"]), c
        assert S.oracle_size(*c["shape"], chosen)[1] == c["color_type"], c
    for key, sizes in t["sizes"].items():
        if key.startswith("300x300"):
            continue
        w, rest = key.split("x")
        h, mode = rest.split("_mode")
        assert [S.oracle_size(int(w), int(h), int(mode), s)[0] for s in range(len(sizes))] == sizes, key

"""The table tests/test_gpu_ssim.py holds pngloss_hip_optimize_batch_target2 to (tests/golden/ssim_target_table.json), from the CPU oracle alone (no
GPU): every image is P.synth_rgba(w, h, mode, 0) at bleed 2 and M = 40, probed with U.run_port, measured with the Python-integer restatement of the
SSIM record (tests/util_ssim.py:py_ssim) and searched with the rule restated in Python.  The two targets, 0.95 and 0.99, were picked here so that
the table holds every kind of outcome: M accepted at once, a search that ends between 0 and M, and an image too small for a window."""
import pytest

from tests import util_distort as D
from tests import util_ssim as S
from tests import util_target as T

TABLE = S.load_table()


@pytest.mark.parametrize("case", TABLE["cases"], ids=lambda c: "min_ssim_%s" % c["min_ssim"])
def test_the_committed_table_is_what_the_rule_gives_on_the_cpu_oracle(case):
    assert TABLE["max_strength"] == S.TABLE_M and [tuple(s) for s in TABLE["shapes"]] == S.TABLE_SHAPES
    for shape, want_chosen, want_seq in zip(S.TABLE_SHAPES, case["chosen"], case["probes"]):
        chosen, seq, margin = S.oracle_search2(shape, S.TABLE_M, case["min_ssim"])
        print(shape, "min_ssim", case["min_ssim"], "->", chosen, seq, "closest SSIM decision:", margin)
        assert (chosen, seq) == (want_chosen, want_seq)
        assert len(seq) <= T.py_probe_bound(S.TABLE_M)
        # the mean is one double division of an exact integer sum: rounding moves it by 1e-16, no decision is nearer than 1e-4
        assert margin is None or margin >= 1e-4


def test_the_table_covers_every_outcome():
    for case in TABLE["cases"]:
        chosen = dict(zip(S.TABLE_SHAPES, case["chosen"]))
        assert any(c == S.TABLE_M for c in chosen.values()) and any(0 < c < S.TABLE_M for c in chosen.values())      # neither all accepted at M nor all 0
        assert chosen[(40, 7, 0)] == S.TABLE_M and S.geometry(40, 7) == (0, 0)      # no window: the SSIM condition does not apply
    a, b = (dict(zip(S.TABLE_SHAPES, c["chosen"])) for c in TABLE["cases"])
    assert a != b and all(b[s] <= a[s] for s in S.TABLE_SHAPES)      # the stricter target never chooses more on these images
    # SSIM is not monotone in the strength either: on 64x16 mode 0 strength 30 keeps more structure than strength 20
    m20, m30 = (S.py_mean(S.oracle_ssim(64, 16, 0, s), D.PSNR_MASK_OF_BPP[T.oracle_probe(64, 16, 0, s)[4]]) for s in (20, 30))
    assert m30 > m20


def test_the_ssim_condition_combines_with_the_others():
    """all set conditions must hold, on 130x9 mode 3 at M = 40: 33 dB alone chooses 31 and a mean SSIM of 0.90 alone 27 -- together 27; 36 dB alone
    chooses 26 -- with 0.90 still 26.  The stricter condition decides."""
    shape = (130, 9, 3)
    assert T.oracle_search(shape, 40, 33.0, 0)[0] == 31 and S.oracle_search2(shape, 40, 0.90)[0] == 27
    assert S.oracle_search2(shape, 40, 0.90, min_psnr_db=33.0)[:2] == (27, [40, 20, 30, 25, 27, 28])
    assert T.oracle_search(shape, 40, 36.0, 0)[0] == 26
    assert S.oracle_search2(shape, 40, 0.90, min_psnr_db=36.0)[:2] == (26, [40, 20, 30, 25, 27, 26])
    assert S.oracle_search2(shape, 40, 0.0, min_psnr_db=33.0)[:2] == T.oracle_search(shape, 40, 33.0, 0)[:2]      # min_ssim = 0: the older rule

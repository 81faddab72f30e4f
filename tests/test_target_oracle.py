"""The fixed cases of tests/test_gpu_target.py, from the CPU oracle alone (no GPU): every case is P.synth_rgba(w, h, mode, 0) at bleed 2, probed with
U.run_port, measured with numpy (tests/util_distort.py) and searched with the rule restated in Python (tests/util_target.py).  The chosen strengths
and probe sequences are pinned here, so the GPU test is known to cover each branch of the search: the probe bound reached, M accepted at once,
nothing accepted, a table that is not monotone, and the largest-error condition alone on a gray image.

Three figures differ from the table of the issue that asked for this test, all by arithmetic and none by choice: (97, 5, 1) at M = 19 with a
60 dB target takes the probes 19, 9, 4, 2, 1 -- five, not six (the rule defines the count, and 1 + ceil(log2 19) = 6 is only its bound); and the
closest decision of the five cases, (130, 6, 3) at strength 32, lies 0.51 dB from its target, not 0.8 dB -- far more than double rounding moves; and of
the strengths 11 and 12 of that image only 11 misses 39 dB (38.44 dB; 12 gives 39.08 dB), which shows the same thing: strength 30 (40.01 dB) distorts less."""
import pytest

from tests import util_distort as D
from tests import util_target as T


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: "%dx%d_mode%d" % c[0])
def test_fixed_case_on_the_cpu_oracle(case):
    shape, m, psnr, max_abs, want_chosen, want_seq = case
    chosen, seq, margin = T.oracle_search(shape, m, psnr, max_abs)
    print(shape, "M", m, "target", psnr, max_abs, "->", chosen, seq, "closest PSNR decision (dB):", margin)
    assert (chosen, seq) == (want_chosen, want_seq)
    assert len(seq) <= T.py_probe_bound(m)
    if margin is not None:
        assert margin >= 0.5                   # rounding in a PSNR cannot flip a decision


def test_the_cases_cover_every_branch():
    by_shape = {c[0]: c for c in T.CASES}
    # the probe bound reached; M accepted at once; nothing accepted (chosen 0 without an accepted probe)
    assert len(by_shape[(64, 8, 0)][5]) == T.py_probe_bound(19) == 6
    assert by_shape[(33, 16, 2)][5] == [19] and by_shape[(33, 16, 2)][4] == 19
    assert by_shape[(97, 5, 1)][4] == 0 and len(by_shape[(97, 5, 1)][5]) == 5
    # not monotone: strengths below the chosen one fail the target the chosen one meets
    w, h, mode = 130, 6, 3
    psnr = {s: D.py_psnr_db(T.oracle_probe(w, h, mode, s)[3], D.PSNR_MASK_OF_BPP[T.oracle_probe(w, h, mode, s)[4]]) for s in (11, 12, 20, 30)}
    print("130x6 mode 3, PSNR by strength:", psnr)
    assert psnr[11] < 39.0 and psnr[20] >= 39.0 and psnr[30] >= 39.0 and psnr[30] > psnr[12] > psnr[11]      # more strength, LESS distortion
    assert psnr[11] == pytest.approx(38.4, abs=0.05) and T.oracle_probe(w, h, mode, 29)[3]["pixels"] == w * h
    # the largest-error condition alone, on an image the optimiser stores as gray: 7 probes for M = 40, the bound
    img, out, _, rec, bpp = T.oracle_probe(64, 8, 4, 8)
    assert bpp == 1 and max(rec["max_abs"]) <= 8 and len(by_shape[(64, 8, 4)][5]) == T.py_probe_bound(40) == 7
    # the images of one batch part ways: the rounds of the five searches hold different strengths
    rounds = [sorted({c[5][r] for c in T.CASES if r < len(c[5])}) for r in range(7)]
    assert [len(r) for r in rounds] == [2, 2, 4, 4, 4, 3, 1]

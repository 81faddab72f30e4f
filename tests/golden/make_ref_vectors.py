"""Record what the REAL reference's builds under oracle/_ref give on the inputs of the CPU tests that compare against them live, so that
those tests still compare against the reference where oracle/_ref is not built.

Run where the reference tree is (oracle/_ref built by `make -C oracle`):   python tests/golden/make_ref_vectors.py

Outputs (data only -- inputs and expected outputs, no reference source in any form):
  tests/golden/seeded_ref.npz       "cNN/out", "cNN/filters": optimize_with_rows on tests.util.seeded_cases(seed=11, n=36)
                                    (inputs are regenerated from the seed, so only outputs are stored)
  tests/golden/rwpng_ref.npz        "<name>.png": the input PNGs of tests/test_cli_host.py:_samples; "expected.json": per input, policy and
                                    strip, the stdout and the sha256 of the file oracle/_ref/rwpng_copy_ref writes
  tests/golden/cli_errors_ref.json  exit code and first stderr line of oracle/_ref/pngloss_ref_cli for test_cli_host.CLI_ERROR_ARGS
"""
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_cli_host as T  # noqa: E402
from tests import util as U  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    assert U.ref() is not None and os.path.exists(T.REF_RWPNG) and os.path.exists(T.REF_CLI), "build oracle/_ref first: make -C oracle"
    arrays = {}
    for i, (img, s, b, filt) in enumerate(U.seeded_cases(seed=11, n=36)):
        out, f = U.run_ref(img, s, b, filt)
        arrays["c%02d/out" % i] = out
        if filt:
            arrays["c%02d/filters" % i] = f
    np.savez_compressed(os.path.join(HERE, "seeded_ref.npz"), **arrays)

    with tempfile.TemporaryDirectory() as tmp:
        d = pathlib.Path(tmp)
        pngs, want = {}, {}
        for src in T._samples(d):
            name = os.path.basename(src)
            pngs[name] = np.frombuffer(open(src, "rb").read(), np.uint8)
            want[name] = []
            for policy in (-1, 0, 1, 2, 3, 4, 5):
                for strip in (0, 1):
                    dst = str(d / "out.png")
                    r = subprocess.run([T.REF_RWPNG, src, dst, str(policy), str(strip)], capture_output=True, text=True, check=True)
                    want[name].append(dict(policy=policy, strip=strip, stdout=r.stdout, sha256=hashlib.sha256(open(dst, "rb").read()).hexdigest()))
        pngs["expected.json"] = np.frombuffer(json.dumps(want).encode(), np.uint8)
        np.savez_compressed(os.path.join(HERE, "rwpng_ref.npz"), **pngs)

        recs = []
        for args in T.CLI_ERROR_ARGS:
            # argv[0] = "pngloss": the tool names itself by argv[0] in some messages, and the recorded lines must not carry where it was built
            r = subprocess.run(["pngloss"] + args, executable=T.REF_CLI, capture_output=True, text=True, cwd=tmp)
            recs.append(dict(args=args, returncode=r.returncode, stderr_first_line=r.stderr.strip().splitlines()[:1]))
    with open(os.path.join(HERE, "cli_errors_ref.json"), "w") as fh:
        json.dump(recs, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Record the complete stderr and the exit code of the -v runs of tests/test_gpu_cli.py:VERBOSE_RUNS from a built pngloss tool.  Needs an MI355X.

Run with the tool to record FROM -- the commit before a change to the tool, never the code under test -- and that commit's name:
    python tests/golden/make_cli_verbose_stderr.py path/to/pngloss COMMIT [output.json]

Output: tests/golden/cli_verbose_stderr.json  {"recorded_from": COMMIT, "runs": [{"args", "returncode", "stderr"}]}"""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_gpu_cli as G  # noqa: E402


def main():
    tool, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden", "cli_verbose_stderr.json")
    with tempfile.TemporaryDirectory() as tmp:
        runs = G.run_verbose(tool, pathlib.Path(tmp))
    with open(out, "w") as fh:
        json.dump(dict(recorded_from=commit, runs=runs), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

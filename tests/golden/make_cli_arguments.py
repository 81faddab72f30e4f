"""Record what a built pngloss tool answers to the argument vectors of tests/test_cli_options_host.py: exit code, full stderr and full stdout.
No vector gets further than opening a file that does not exist, so no device is needed.

Run with the tool to record FROM -- the commit before a change to the tool's argument handling, never the code under test:
    python tests/golden/make_cli_arguments.py path/to/pngloss

Output: tests/golden/cli_arguments.json  {"library_version": the library's name for itself inside the version banner (the one part of the recorded
text that changes with the library, not with the tool), "vectors": [{"args", "returncode", "stderr", "stdout"}]}"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
X = ["x.png"]

#: the twelve reference-era vectors (tests/test_cli_host.py:CLI_ERROR_ARGS)
REFERENCE_ERA = [[], ["-s", "300"] + X, ["-b", "0"] + X, ["-b", "40000"] + X, ["-s", "abc"] + X, ["-o", "a.png", "-o", "b.png"] + X,
                 ["--ext", "e.png", "-o", "a.png"] + X, ["-o", "a.png", "x.png", "y.png"], ["-o", "-", "x.png", "y.png"], ["--bogus"],
                 ["-f", "/nonexistent/dir/file.png"], ["-V"]]
#: one per rule added since: values that do not parse, values out of range, combinations that are refused
RULES = [["--target-psnr", "x"], ["--max-error", "x"], ["--target-ssim", "x"], ["-b", "x"],
         ["--target-size", "5q"], ["--target-size", "99999999999999999999"], ["--target-size", "18014398509481984k"], ["--target-size", "17592186044416M"],
         ["--target-psnr", "-1"], ["--target-psnr", "nan"], ["--target-ssim", "0"], ["--target-ssim", "2"], ["--max-error", "0"], ["--max-error", "256"],
         ["--target-size", "10k", "--target-psnr", "40"], ["--target-size", "10k", "--max-error", "3"], ["--target-size", "10k", "--target-ssim", "0.9"],
         ["--visible"], ["--visible", "--distortion", "--target-size", "5k"], ["--target-size", "0"], ["--target-size", "0%"],
         ["--indexed", "--target-size", "10k"], ["--indexed", "--target-psnr", "40"], ["--indexed", "--target-ssim", "0.9"], ["--indexed", "--max-error", "3"]]
#: several rules broken at once: the message is that of the first in the order of the checks
ORDER = [["-s", "300", "--target-ssim", "2"], ["--target-psnr", "40", "-b", "0"], ["--target-size", "10k", "--target-psnr", "-1"],
         ["--visible", "--target-size", "5k"], ["--indexed", "--visible"], ["--ext", "e.png", "-o", "a.png", "--target-size", "0"],
         ["--target-ssim", "2", "--max-error", "0"], ["--max-error", "0", "--target-size", "10k"], ["--indexed", "--target-size", "0"],
         ["--indexed", "--target-psnr", "40", "-b", "0"], ["-b", "0", "--ext", "e.png", "-o", "a.png"], ["-s", "300", "-s", "abc"]]
#: vectors that pass every rule: the tool goes on to x.png, which does not exist
VALID = [[], ["--target-size", "10k"], ["--target-size", "50%", "-s", "40", "--distortion", "--ssim"], ["--target-psnr", "40"], ["--max-error", "3"],
         ["--target-ssim", "0.9", "--ssim", "--visible"], ["--target-psnr", "35", "--max-error", "8", "--target-ssim", "1"], ["--indexed"],
         ["--visible", "--distortion"], ["--gpu-deflate", "--gpu-read", "-f", "--strip", "--skip-if-larger", "--ext", ".e.png", "y.png"],
         ["-s", "0", "-b", "32767"], ["-s", "255", "-b", "1", "-f", "--no-force"], ["-v", "-q"], ["-o", "out.png"]]

VECTORS = (REFERENCE_ERA + [v + X for v in RULES + ORDER + VALID] +
           [["--help"], ["-q", "-v"], ["-o", "-", "x.png"], ["-"], ["-o", "out.png", "-"], ["--", "-s"]])


def run(tool, args, cwd):
    """argv[0] = "pngloss": getopt_long names the program in its own messages, and the recorded text must not carry where the tool was built"""
    return subprocess.run(["pngloss"] + args, executable=tool, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def main():
    tool = os.path.abspath(sys.argv[1])
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for args in VECTORS:
            r = run(tool, args, tmp)
            assert not os.listdir(tmp), args
            recs.append(dict(args=args, returncode=r.returncode, stderr=r.stderr, stdout=r.stdout))
        banner = run(tool, ["--help"], tmp).stdout
    version = re.match(r"pngloss, \S+, filter\+quantise path on AMD MI355X \((.*)\)\.\n", banner).group(1)
    with open(os.path.join(HERE, "cli_arguments.json"), "w") as fh:
        json.dump(dict(library_version=version, vectors=recs), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

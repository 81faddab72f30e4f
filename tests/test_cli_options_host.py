"""CPU tests of what the command line tool decides without I/O (no GPU, no libpng for the drivers):
  * pngloss_amd/cli/cli_options.c -- the command line, parsed and checked -- on its own (tests/c/cli_options_host.c) and inside the built tool, over
    argument vectors whose answers were recorded from the tool as it was BEFORE the options moved into a file of their own
    (tests/golden/cli_arguments.json, written by tests/golden/make_cli_arguments.py): exit code, full stderr, full stdout.  One vector per rule,
    and vectors that break several rules, which pin the order of the checks;
  * pngloss_amd/cli/cli_outcome.h -- what a library answer means for one file -- over its whole domain (tests/c/cli_outcome_host.c), against tables
    written out here from the rules, and against a restatement of the expressions those functions replaced."""
import itertools
import json
import os
import subprocess

import pytest

import pngloss_amd as P
from pngloss_amd import lib as L
from tests import util as U

CLI = os.path.join(U.ROOT, "pngloss_amd", "cli")
have_png = os.path.exists("/opt/conda/include/png.h") and os.path.exists("/lib/x86_64-linux-gnu/libpng16.so.16")
needs_tool = pytest.mark.skipif(not have_png, reason="libpng headers/runtime not found on this box: the command line tool is not built")
OK, ABORT, HIP, OOM, INVALID = L.PNGLOSS_SUCCESS, L.PNGLOSS_INTERNAL_ABORT, L.PNGLOSS_HIP_ERROR, L.PNGLOSS_OUT_OF_MEMORY_ERROR, L.PNGLOSS_INVALID_ARGUMENT
CODES = (OK, ABORT, HIP, OOM)


def _recorded():
    with open(os.path.join(U.GOLDEN, "cli_arguments.json")) as fh:
        return json.load(fh)


def _gcc(out, source, *more):
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I" + CLI, "-o", out, os.path.join(U.ROOT, "tests", "c", source)] + list(more),
                   check=True, capture_output=True)
    return out


@pytest.fixture(scope="module")
def options_host(tmp_path_factory):
    """cli_options.c and nothing else: no libpng, no device library"""
    return _gcc(str(tmp_path_factory.mktemp("cli_options") / "cli_options_host"), "cli_options_host.c", os.path.join(CLI, "cli_options.c"))


@pytest.fixture(scope="module")
def outcome_host(tmp_path_factory):
    return _gcc(str(tmp_path_factory.mktemp("cli_outcome") / "cli_outcome_host"), "cli_outcome_host.c")


def _run(exe, args, cwd):
    """argv[0] = "pngloss", as the recorder ran the tool: getopt_long names the program in its own messages"""
    return subprocess.run(["pngloss"] + args, executable=exe, capture_output=True, text=True, cwd=cwd, stdin=subprocess.DEVNULL)


def _fields(stdout):
    return dict(line.split("=", 1) for line in stdout.splitlines())


# ---- the argument matrix ----

def test_recording_holds_the_vectors_and_the_messages_seen_on_the_tool_before_the_move():
    rec = {tuple(v["args"]): v for v in _recorded()["vectors"]}
    x = ("x.png",)
    from tests.test_cli_host import CLI_ERROR_ARGS
    assert all(tuple(a) in rec for a in CLI_ERROR_ARGS)
    seen = {("--target-size", "10k", "--target-psnr", "40") + x: "--target-size cannot be combined with --target-psnr, --target-ssim or --max-error.\n",
            ("--target-size", "10k", "--max-error", "3") + x: "--target-size cannot be combined with --target-psnr, --target-ssim or --max-error.\n",
            ("--visible",) + x: "--visible needs one of --distortion, --ssim, --target-psnr, --max-error or --target-ssim.\n",
            ("--visible", "--target-size", "5k") + x: "--visible needs one of --distortion, --ssim, --target-psnr, --max-error or --target-ssim.\n",
            ("--indexed", "--visible") + x: "--visible needs one of --distortion, --ssim, --target-psnr, --max-error or --target-ssim.\n",
            ("--visible", "--distortion", "--target-size", "5k") + x: "--visible cannot be combined with --target-size.\n",
            ("--target-size", "0") + x: "Must specify a size target of at least 1 byte or 1 percent.\n",
            ("--target-size", "0%") + x: "Must specify a size target of at least 1 byte or 1 percent.\n",
            ("--ext", "e.png", "-o", "a.png", "--target-size", "0") + x: "Must specify a size target of at least 1 byte or 1 percent.\n",
            ("-s", "300", "--target-ssim", "2") + x: "Must specify a strength in the range 0-255.\n",
            ("--target-psnr", "40", "-b", "0") + x: "Must specify a bleed divider in the range 1-32767.\n",
            ("--target-size", "10k", "--target-psnr", "-1") + x: "Must specify a PSNR target of 0 dB or more.\n",
            ("--target-psnr", "nan") + x: "Must specify a PSNR target of 0 dB or more.\n",
            ("--target-ssim", "0") + x: "Must specify an SSIM target above 0 and at most 1.\n",
            ("--target-ssim", "2") + x: "Must specify an SSIM target above 0 and at most 1.\n",
            ("--max-error", "0") + x: "Must specify a largest channel error in the range 1-255.\n",
            ("--max-error", "256") + x: "Must specify a largest channel error in the range 1-255.\n",
            ("--target-psnr", "x") + x: "--target-psnr requires a numeric argument\n"}
    for value in ("5q", "99999999999999999999", "18014398509481984k"):
        seen[("--target-size", value) + x] = "--target-size requires a number of bytes (suffix k or M) or a percentage\n"
    for other in (("--target-size", "10k"), ("--target-psnr", "40"), ("--target-ssim", "0.9"), ("--max-error", "3")):
        seen[("--indexed",) + other + x] = "--indexed cannot be combined with --target-size, --target-psnr, --target-ssim or --max-error.\n"
    for args, message in seen.items():
        assert (rec[args]["returncode"], rec[args]["stderr"], rec[args]["stdout"]) == (INVALID, message, ""), args
    assert rec[("-V",)]["returncode"] == 0 and rec[("--help",)]["returncode"] == 0 and rec[("--help",)]["stdout"].startswith("pngloss, ")
    assert rec[()]["returncode"] == 1 and rec[("-q", "-v")]["returncode"] == 1 and rec[("-q", "-v")]["stderr"].startswith("No input files specified.\npngloss, ")


def test_options_on_their_own_answer_like_the_recorded_tool(options_host, tmp_path):
    """every refused vector: the recorded message and code, byte for byte.  The others pass the check; what the tool answers before the check
    (--version, --help, no arguments) shows in the record"""
    for v in _recorded()["vectors"]:
        r = _run(options_host, v["args"], tmp_path)
        if v["returncode"] == INVALID:
            assert (r.returncode, r.stderr, r.stdout) == (INVALID, v["stderr"], ""), v["args"]
        elif v["args"] == ["-q", "-v"]:      # the tool goes on with the version banner (-v) and the usage text
            assert (r.returncode, r.stderr, r.stdout) == (1, "No input files specified.\n", "") and v["stderr"].startswith(r.stderr)
        else:
            assert r.returncode == 0 and r.stderr == "", (v["args"], r.stderr)
            f = _fields(r.stdout)
            assert (f["version"], f["help"], f["missing"]) == (str(int(v["args"] == ["-V"])), str(int(v["args"] == ["--help"])), str(int(not v["args"]))), v["args"]
    assert not os.listdir(tmp_path)


@needs_tool
def test_built_tool_answers_like_the_recorded_tool(tmp_path):
    """exit code, full stderr and full stdout of every vector.  The version banner names the library by pngloss_hip_version(): that part of the
    recorded text follows the library"""
    exe = os.path.join(CLI, "pngloss")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CLI], check=True, capture_output=True)
    rec = _recorded()
    now = P.hip_lib().pngloss_hip_version().decode()
    for v in rec["vectors"]:
        r = _run(exe, v["args"], tmp_path)
        want = (v["returncode"], v["stderr"].replace(rec["library_version"], now), v["stdout"].replace(rec["library_version"], now))
        assert (r.returncode, r.stderr, r.stdout) == want, v["args"]
    assert not os.listdir(tmp_path)


DEFAULTS = dict(extension="", output_path="", files="x.png", strength="19", bleed="2", num_files="1", from_stdin="0", to_stdout="0", force="0", skip_if_larger="0",
                strip="0", help="0", version="0", missing="0", verbose="0", gpu_deflate="0", gpu_read="0", distortion="0", ssim="0", visible="0", indexed="0",
                search="none", target_psnr="0", have_max_error="0", max_error="0", have_target_ssim="0", target_ssim="0", size_percent="0", size_value="0")
X = ["x.png"]
#: (command line; the fields that differ from DEFAULTS)
VALID = [(X, {}),
         (["--target-size", "10k"] + X, dict(search="size", gpu_deflate="1", size_value="10240")),
         (["--target-size", "3M", "--gpu-deflate"] + X, dict(search="size", gpu_deflate="1", size_value=str(3 << 20))),
         (["--target-size", "50%", "-s", "40", "--distortion", "--ssim"] + X, dict(search="size", gpu_deflate="1", size_value="50", size_percent="1", strength="40", distortion="1", ssim="1")),
         (["--target-psnr", "40"] + X, dict(search="quality", target_psnr="40")),
         (["--max-error", "3"] + X, dict(search="quality", have_max_error="1", max_error="3")),
         (["--target-ssim", "0.9", "--ssim", "--visible"] + X, dict(search="quality", have_target_ssim="1", target_ssim="0.90000000000000002", ssim="1", visible="1")),
         (["--target-psnr", "35", "--max-error", "8", "--target-ssim", "1"] + X, dict(search="quality", target_psnr="35", have_max_error="1", max_error="8", have_target_ssim="1", target_ssim="1")),
         (["--indexed"] + X, dict(indexed="1", gpu_deflate="1")),
         (["--visible", "--distortion"] + X, dict(visible="1", distortion="1")),
         (["--gpu-deflate", "--gpu-read", "-f", "--strip", "--skip-if-larger", "--ext", ".e.png", "y.png"] + X,
          dict(gpu_deflate="1", gpu_read="1", force="1", strip="1", skip_if_larger="1", extension=".e.png", files="y.png x.png", num_files="2")),
         (["-s", "255", "-b", "1", "-f", "--no-force"] + X, dict(strength="255", bleed="1")),
         (["-v", "-q"] + X, {}), (["-q", "-v"] + X, dict(verbose="1")),
         (["-o", "out.png"] + X, dict(output_path="out.png")),
         (["-o", "-"] + X, dict(to_stdout="1")),
         (["-"], dict(files="-", from_stdin="1", to_stdout="1")),
         (["-o", "out.png", "-"], dict(files="-", from_stdin="1", output_path="out.png")),
         (["--", "-s"], dict(files="-s"))]


@pytest.mark.parametrize("args,differs", VALID, ids=[" ".join(a) for a, _ in VALID])
def test_valid_vectors_give_the_record(options_host, tmp_path, args, differs):
    """the search mode is derived once, --indexed and --target-size imply --gpu-deflate, a lone "-" is the pipe"""
    r = _run(options_host, args, tmp_path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert _fields(r.stdout) == dict(DEFAULTS, **differs)


# ---- what a library answer means for one file ----

def _grid(outcome_host, kind):
    out = subprocess.run([outcome_host], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines() if line.startswith(kind + " ")]
    return {tuple(int(t) for t in row[1:row.index("->")]): tuple(int(t) for t in row[row.index("->") + 1:]) for row in rows}


def test_status_after_the_optimise_call(outcome_host):
    """a failure unless the call succeeded, or it returned PNGLOSS_INTERNAL_ABORT and this image's status is 0"""
    want = {(OK, 0): (0,), (OK, ABORT): (0,), (ABORT, 0): (0,), (ABORT, ABORT): (ABORT,),
            (HIP, 0): (HIP,), (HIP, ABORT): (HIP,), (OOM, 0): (OOM,), (OOM, ABORT): (OOM,)}
    assert _grid(outcome_host, "optimise") == want
    for (rc, st), (got,) in want.items():        # the expression this replaced: `if (rc != SUCCESS && !(rc == INTERNAL_ABORT && res[k].status == 0)) status = rc`
        assert got == (rc if rc != OK and not (rc == ABORT and st == 0) else 0)


#: with the switch on -- (search, return code, pngloss_hip_multi_last_* succeeded): (distortion, SSIM with --target-ssim, SSIM without it, palette).
#: The plain call's records are in the context: valid where last_* gave them.  A search's are in its reports, filled when it returns success or
#: PNGLOSS_INTERNAL_ABORT; the quality search has an SSIM record only with --target-ssim, the size search none, and neither a palette.
NONE, QUALITY, SIZE = 0, 1, 2
RECORDS = {(NONE, OK, 1): (1, 1, 1, 1), (NONE, ABORT, 1): (1, 1, 1, 1), (NONE, HIP, 1): (1, 1, 1, 1), (NONE, OOM, 1): (1, 1, 1, 1),
           (NONE, OK, 0): (0, 0, 0, 0), (NONE, ABORT, 0): (0, 0, 0, 0), (NONE, HIP, 0): (0, 0, 0, 0), (NONE, OOM, 0): (0, 0, 0, 0),
           (QUALITY, OK, 1): (1, 1, 0, 0), (QUALITY, ABORT, 1): (1, 1, 0, 0), (QUALITY, HIP, 1): (0, 0, 0, 0), (QUALITY, OOM, 1): (0, 0, 0, 0),
           (QUALITY, OK, 0): (1, 1, 0, 0), (QUALITY, ABORT, 0): (1, 1, 0, 0), (QUALITY, HIP, 0): (0, 0, 0, 0), (QUALITY, OOM, 0): (0, 0, 0, 0),
           (SIZE, OK, 1): (1, 0, 0, 0), (SIZE, ABORT, 1): (1, 0, 0, 0), (SIZE, HIP, 1): (0, 0, 0, 0), (SIZE, OOM, 1): (0, 0, 0, 0),
           (SIZE, OK, 0): (1, 0, 0, 0), (SIZE, ABORT, 0): (1, 0, 0, 0), (SIZE, HIP, 0): (0, 0, 0, 0), (SIZE, OOM, 0): (0, 0, 0, 0)}


def _records_before(have_size, have_target, have_target_ssim, asked, rc, last_ok):
    """the three-branch block of the tool's result loop as it was, with one switch value for --distortion, --ssim and --indexed"""
    if have_size:
        return asked and rc in (OK, ABORT), False, False
    if have_target:
        return asked and rc in (OK, ABORT), asked and have_target_ssim and rc in (OK, ABORT), False
    return asked and last_ok, asked and last_ok, asked and last_ok


def test_which_records_are_valid(outcome_host):
    got = _grid(outcome_host, "records")
    assert len(got) == 3 * 2 * 2 * 4 * 2
    for search, asked, tssim, rc, last in itertools.product((NONE, QUALITY, SIZE), (0, 1), (0, 1), CODES, (0, 1)):
        d, s_with, s_without, p = RECORDS[(search, rc, last)] if asked else (0, 0, 0, 0)
        assert got[(search, asked, tssim, rc, last)] == (d, s_with if tssim else s_without, p), (search, asked, tssim, rc, last)
        before = _records_before(search == SIZE, search == QUALITY, bool(tssim), bool(asked), rc, bool(last))
        assert got[(search, asked, tssim, rc, last)] == tuple(int(v) for v in before)
    # an indexed stream (colour type 3) without its palette is an error of its own only where the call succeeded
    assert _grid(outcome_host, "indexed") == {(t, have, rc): (int(t == 3 and not have and rc == OK),) for t in (3, 6) for have in (0, 1) for rc in CODES}


def test_status_after_the_device_read(outcome_host):
    """(setup code, batch code, this file's status, some file's status explains the batch code): a setup failure goes to every file; else the
    file's own status; else the batch code where no status explains it -- never a file taken for decoded on the strength of its 0 alone"""
    st = INVALID
    want = {(OK, OK, 0, 0): 0, (OK, OK, 0, 1): 0, (OK, OK, st, 0): st, (OK, OK, st, 1): st,
            (OK, HIP, 0, 0): HIP, (OK, HIP, 0, 1): 0, (OK, HIP, st, 0): st, (OK, HIP, st, 1): st,
            (OOM, OK, 0, 0): OOM, (OOM, OK, 0, 1): OOM, (OOM, OK, st, 0): OOM, (OOM, OK, st, 1): OOM,
            (OOM, HIP, 0, 0): OOM, (OOM, HIP, 0, 1): OOM, (OOM, HIP, st, 0): OOM, (OOM, HIP, st, 1): OOM}
    got = _grid(outcome_host, "read")
    assert got == {k: (v,) for k, v in want.items()}
    assert got[(OK, HIP, 0, 0)] != (0,)          # the case the comment warns about
    for (rc, brc, one, explained), (code,) in got.items():       # `one = rc != OK ? rc : (st[q] ? st[q] : ((brc != OK && !explained) ? brc : OK))`
        assert code == (rc if rc != OK else (one if one else (brc if brc != OK and not explained else OK)))


def test_size_budget_of_one_file(outcome_host):
    def budget(percent, value, size):
        return int(subprocess.run([outcome_host, "budget", str(percent), str(value), str(size)], capture_output=True, text=True, check=True).stdout)

    def stream(largest):
        return int(subprocess.run([outcome_host, "stream", str(largest)], capture_output=True, text=True, check=True).stdout)

    assert budget(1, 50, 1001) == 500                                   # percent, rounded down
    assert budget(1, 1, 10) == 1 and budget(1, 0, 10) == 1              # the floor of 1 byte
    assert budget(1, 250, 1000) == 2500 and budget(1, 100, 12345) == 12345
    assert budget(0, 4096, 10) == 4096 and budget(0, 1, 10 ** 6) == 1   # bytes pass through, whatever the input's size
    for percent, value, size in ((1, 50, 1001), (1, 1, 10), (1, 33, 10 ** 9 + 7), (0, 4096, 10)):    # the tool's expression as it was, in integers
        assert budget(percent, value, size) == max(1, size * value // 100 if percent else value)
    assert stream(0) == 1 and stream(1) == 1 and stream(12345) == 12345   # a container that leaves no room: 1 byte, which no stream meets

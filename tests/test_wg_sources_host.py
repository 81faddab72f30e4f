"""The sources of the workgroup engine (pngloss_amd/csrc/pl_engine.hip and its parts pl_wg_*.h): the generated header is what its generator prints, and the
switches and macros that were removed stay out."""
import glob
import os
import subprocess
import sys

from tests import util as U

CSRC = os.path.join(U.ROOT, "pngloss_amd", "csrc")


def sources():
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if f.endswith((".hip", ".h", ".c")) or os.path.basename(f) == "Makefile")
    assert len(files) > 40
    return {os.path.basename(f): open(f).read() for f in files}


def test_the_generated_loops_are_what_the_generator_prints():
    """pl_lead_asm.h is tools/gen_lead_asm.py's output under its default settings (no PL_LEAD_* variable set)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PL_LEAD_")}
    r = subprocess.run([sys.executable, os.path.join(U.ROOT, "tools", "gen_lead_asm.py")], capture_output=True, text=True, env=env, check=True)
    assert r.stdout == open(os.path.join(CSRC, "pl_lead_asm.h")).read()


def test_the_removed_switches_stay_out():
    for name, text in sources().items():
        assert "PL_ABLATE" not in text and "PL_PREFETCH_FIX" not in text, name


def test_no_offset_macro_beside_the_layout_table():
    """the LDS carve-up of pl_engine is pl_wg_lds.h's table: no PL_SM_* macro states an offset anywhere else"""
    src = sources()
    for name, text in src.items():
        assert "PL_SM_" not in text, name
    assert '#include "pl_wg_lds.h"' in src["pl_engine.hip"] and "PL_WG_LAUNCH_BYTES" in src["pl_engine.hip"]
    # the engine's parts are included by pl_engine.hip, in the order a row goes through them
    at = [src["pl_engine.hip"].index('#include "%s"' % h) for h in ("pl_wg_util.h", "pl_wg_chain.h", "pl_wg_lead.h", "pl_wg_post.h")]
    assert at == sorted(at)
    assert '#include "pl_lead_asm.h"' in src["pl_wg_lead.h"]

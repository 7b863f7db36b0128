"""The host-side planning of the search path (merizo_search_amd/csrc/ms_plan.h) on a CPU: tests/c_abi/plan_fingerprint.cpp is built
with the host compiler, without HIP, and run once.  Its plans and workspace layouts must be the ones recorded in
tests/golden/plan_fingerprints.txt (from the planning code as it stood before it moved into the header), every carved region must
be aligned, disjoint, inside the workspace and large enough for its writers, and the table of switches must be the documented one."""
import hashlib
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "merizo_search_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "c_abi", "plan_fingerprint.cpp"), os.path.join(CSRC, "ms_plan.h"),
           os.path.join(ROOT, "include", "merizo_search_amd.h")]

# name -> default: every environment variable of the search path ("Switches of the search path")
SWITCHES = {
    "MS_LOADER_WAVE": "1", "MS_HEAD_MERGE": "1", "MS_BLOCK_MERGE": "1", "MS_LIST_SM": "1", "MS_SHARED_BOUND": "1",
    "MS_PREPASS_TILES": "-1", "MS_SAMPLE_MIN_NQ": "8", "MS_SAMPLE_COEF": "0.05", "MS_PF_SAMPLE_COEF": "1.2", "MS_BOUND_RANKS": "0",
    "MS_FUSED_MERGE_MAX_NQ": "2", "MS_INKERNEL_NORM_MAX_NQ": "4", "MS_PREFILTER": "1", "MS_PF_FEW_MIN_ROWS": "1000000",
    "MS_PF_FEW2_MIN_ROWS": "200000", "MS_PF_PACE": "1", "MS_PF_RAWQ": "1", "MS_PF_FUSE_EXACT_MAX_NQ": "8", "MS_PF_DEBUG": "0",
}


def _program() -> str:
    base = os.environ.get("MS_TEST_CACHE") or os.path.join(tempfile.gettempdir(), "merizo_search_amd_%d" % os.getuid())
    os.makedirs(base, exist_ok=True)
    digest = hashlib.sha256(b"".join(open(p, "rb").read() for p in SOURCES)).hexdigest()[:16]
    exe = os.path.join(base, "plan_fingerprint_%s" % digest)
    if not os.path.exists(exe):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", tmp, SOURCES[0]], check=True)
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def run():
    return subprocess.run([_program()], capture_output=True, text=True)


def test_plans_and_layouts_match_the_recorded_ones(run):
    got = [ln for ln in run.stdout.splitlines() if ln.startswith(("plan ", "total "))]
    want = open(os.path.join(ROOT, "tests", "golden", "plan_fingerprints.txt")).read().splitlines()
    assert len(want) == 8 * 2 * 14 + 14 * 14
    assert got == want


def test_carved_regions_are_aligned_disjoint_and_large_enough(run):
    # (checked case by case inside the program, which also holds ms_plan_core against make_plan: a finding is a line on stderr)
    assert run.stderr == ""
    assert run.returncode == 0


def test_every_switch_is_in_the_table_with_its_default(run):
    rows = [ln.split()[1:] for ln in run.stdout.splitlines() if ln.startswith("setting ")]
    assert {r[0]: r[1] for r in rows} == SWITCHES                 # the table: names and defaults
    assert all(r[2] == r[1] for r in rows)                        # an unset variable gives the default
    assert all(r[3] == "3" for r in rows)                         # each name is recognised
    # the search path reads its environment in one place (the encoder's MS_EGNN_SPLIT is ms_egnn.hip's own)
    reads = {}
    for name in sorted(os.listdir(CSRC)):
        if name.startswith(("ms_search", "ms_scan", "ms_plan", "ms_common", "ms_topk")):
            reads[name] = len(re.findall(r"\bgetenv\b", open(os.path.join(CSRC, name)).read()))
    assert {k: v for k, v in reads.items() if v} == {"ms_plan.h": 1}
    # and DESIGN.md documents every one of them, default included
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, default in SWITCHES.items():
        assert re.search(r"^\| `%s` \| %s \|" % (name, re.escape(default)), design, re.M), name

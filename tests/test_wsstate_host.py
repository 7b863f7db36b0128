"""The per-workspace records of the search path (merizo_search_amd/csrc/ms_wsstate.h) on a CPU: tests/c_abi/wsstate_check.cpp is built
with the host compiler, without HIP, as a stand-alone program -- once with the address and undefined-behaviour sanitizers, once with the
thread sanitizer -- and run.  The program defines the three device functions the header declares over calloc and call counters, and checks
the table's rules (one record per workspace and device, the least recently used record of the caller's device changes hands and starts
over, tickets advance on commit only, clean counters are taken once, epochs are never 0, threads keep the totals): a finding is a line
on its stderr, and so is anything a sanitizer reports."""
import hashlib
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "c_abi", "wsstate_check.cpp"), os.path.join(ROOT, "merizo_search_amd", "csrc", "ms_wsstate.h")]
SANITIZERS = {"asan_ubsan": "-fsanitize=address,undefined", "tsan": "-fsanitize=thread"}


def _program(name: str) -> str:
    base = os.environ.get("MS_TEST_CACHE") or os.path.join(tempfile.gettempdir(), "merizo_search_amd_%d" % os.getuid())
    os.makedirs(base, exist_ok=True)
    digest = hashlib.sha256(b"".join(open(p, "rb").read() for p in SOURCES)).hexdigest()[:16]
    exe = os.path.join(base, "wsstate_check_%s_%s" % (name, digest))
    if not os.path.exists(exe):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", SANITIZERS[name], "-fno-sanitize-recover=undefined",
                        "-o", tmp, SOURCES[0]], check=True)
        os.replace(tmp, exe)
    return exe


@pytest.mark.parametrize("name", sorted(SANITIZERS))
def test_workspace_records_keep_their_rules(name):
    run = subprocess.run([_program(name)], capture_output=True, text=True)
    assert run.stderr == ""
    assert run.returncode == 0
    assert int(run.stdout.split()[1]) > 700          # (every check ran: the table's capacity alone gives several hundred)

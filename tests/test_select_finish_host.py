"""Host side of the selections' finish (csrc/select.hpp: sel_rank_vote, the self-cleaning histogram): builds tests/diag/select_finish_host_check.hip,
a stand-alone program, with hipcc and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_finish_host_check(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "select_finish_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "diag", "select_finish_host_check.hip")], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "select finish host check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]

"""The dispatch plan of the Kalman log-likelihood kernels (csrc/dsge_kalman_plan.hpp), checked on the host: tests/host/
kalman_plan_check.cpp asserts the instance lists of named shapes and the plan's properties over a sweep of shapes, hints and
options.  The program calls no HIP function and needs no GPU; it is compiled host-only and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_kalman_plan_named_shapes_and_properties(tmp_path):
    exe = str(tmp_path / "kalman_plan_check")
    build = subprocess.run([_hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-I", "geconpy_amd/csrc", "-o", exe,
                            "tests/host/kalman_plan_check.cpp"], cwd=ROOT, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "plans swept, 0 checks failed" in run.stdout

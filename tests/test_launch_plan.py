"""The launch plan (upe_amd/csrc/upe_plan.h: which classify variant, how much LDS for what, the
tiling and grid, the ring stamps, the group-by's shape) on the CPU: `make plan-check` builds
tools/plan_check.cpp, a stand-alone program of hand-derived cases, under the host sanitizers and
runs it.  Nothing is loaded into Python."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "upe_amd", "csrc"), "plan-check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_check: the launch plan agrees" in r.stdout

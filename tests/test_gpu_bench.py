"""A plain bench.py run end to end on the GPU (small batch, 3 steps): the line's contract fields,
no leg beside `value`, --steps honoured, and the --dump-outputs arrays equal to the oracle's
verdicts and rewritten frames of the last step for the same seeded workload."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from upe_amd import gpu, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("other_mode", "imix", "imix_seed3", "imix_v6fwd", "strong", "ring", "egress",
             "config_d", "workers_sharing_gpu", "host_roundtrip", "host_roundtrip_emit",
             "host_mapped", "host_mapped_emit", "cpu_baseline", "dropin_pipeline")


def test_plain_run_line_and_dump(tmp_path):
    n = 20_000   # no multiple of 64, more than one workgroup's chunks
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--packets", str(n), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "Mpps" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["metric"].startswith("Mpps parse+classify")
    assert (d["steps"], d["warmup"], d["n_gpus"]) == (3, 1, 1)
    assert d["ms_per_step"] > 0
    # (both figures are rounded: ms_per_step to 1e-5 ms, value to 0.01 Mpps)
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3) / 1e6,
                                       rel=0.5e-5 / d["ms_per_step"] + 1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["roofline"]["achievable"] is None

    # the workload bench.py builds for rank 0, through the warm-up and the timed steps in order:
    # every step reads a pristine copy of the batch, the worker's L1 state carries on (a verdict
    # word says whether the L1 cache hit)
    wl = synth.config_b(n=n, seed=2)
    l1 = None
    for _ in range(1 + 3):
        ref = oracle.run_restated(wl, l1=l1)
        l1 = ref.l1
    assert sorted(os.listdir(out)) == ["records.npy", "verdict.npy"]
    verdict = np.load(out / "verdict.npy")
    records = np.load(out / "records.npy")
    assert verdict.dtype == records.dtype == np.float64 and records.shape == (n, 4)
    assert d["dumped_outputs"]["arrays"] == {"verdict": [n], "records": [n, 4]}
    assert np.array_equal(verdict.astype(np.uint32), ref.verdict)
    rec = records.astype("<u4").view(np.uint8).reshape(-1, 16)
    assert np.array_equal(gpu.hdr_apply(wl.frames, wl.desc, rec), ref.frames)

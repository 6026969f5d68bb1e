"""bench.py's command line and --dump-outputs on the CPU: a plain run has every leg beside
`value` switched off, --full leaves them as the options say, and dump_outputs writes the last
step's verdicts and per-packet records (emit) or frame heads (inplace) as float arrays under
64 MB, never the record slots the kernel leaves unwritten, with a fixed sample of a batch too
large to dump whole.  The buffers here are CPU tensors filled from the golden vectors; the GPU
side is tests/test_gpu_bench.py."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import bench
import golden_io
from test_emit_records import records_from_reference
from upe_amd import gpu
from upe_amd.layout import REWRITE_EXTENT, V_FWD, desc_lens, desc_offsets

LIMIT = 64 * 1000 * 1000


def _load_dir(path) -> dict:
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _compacted(rec: np.ndarray, verdict: np.ndarray) -> np.ndarray:
    """The emit kernel's buffer: records of forwarded packets compacted per 64-packet group,
    every other slot holding whatever was there before (0xAA here)."""
    raw = np.full((len(verdict), 16), 0xAA, np.uint8)
    fwd = (verdict & 0xF) == V_FWD
    raw[gpu.record_slots(verdict)[fwd]] = rec[fwd]
    return raw


def test_plain_run_has_no_other_leg():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--workers-per-gpu", "4"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_other_mode and a.no_imix and a.no_hbm_probe and a.no_cpu_baseline
    assert (a.strong, a.ring, a.config_d_steps, a.host_reps, a.workers_per_gpu) == (0, 0, 0, 0, 0)


def test_full_run_keeps_the_legs():
    a = bench.parse_args(["--full", "--dump-outputs", "d", "--ring", "8", "--no-imix"])
    assert a.full and a.dump_outputs == "d" and a.no_imix
    assert not (a.no_other_mode or a.no_hbm_probe or a.no_cpu_baseline)
    assert (a.strong, a.ring, a.config_d_steps, a.host_reps) == (1, 8, 20, 5)


@pytest.mark.parametrize("case", ["config_b_small", "config_c_small"])
def test_dump_emit(case, tmp_path):
    wl, ref = golden_io.load(case)
    v = ref["verdict"].astype(np.uint32)
    rec = records_from_reference(wl.frames, ref["frames"], wl.desc, v)
    hdr = torch.from_numpy(_compacted(rec, v).reshape(-1))
    shapes = bench.dump_outputs(torch, str(tmp_path), 0, "emit", wl, v, hdr, None)
    got = _load_dir(tmp_path)
    assert sorted(got) == ["records", "verdict"] == sorted(shapes)
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["verdict"].astype(np.uint32), v)
    words = got["records"].astype("<u4")
    assert np.array_equal(words.view(np.uint8).reshape(-1, 16), rec)
    assert sum(a.nbytes for a in got.values()) <= LIMIT


def test_dump_inplace(tmp_path):
    wl, ref = golden_io.load("config_c_small")
    v = ref["verdict"].astype(np.uint32)
    bench.dump_outputs(torch, str(tmp_path), 1, "inplace", wl, v, None,
                       torch.from_numpy(ref["frames"].copy()))
    got = _load_dir(tmp_path)
    assert sorted(got) == ["frames_rank1", "verdict_rank1"]
    assert got["frames_rank1"].dtype == np.float32
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    for i in list(range(0, wl.n, 97)) + [wl.n - 1]:
        k = min(int(lens[i]), REWRITE_EXTENT)
        want = np.zeros(REWRITE_EXTENT, np.float32)
        want[:k] = ref["frames"][int(offs[i]):int(offs[i]) + k]
        assert np.array_equal(got["frames_rank1"][i], want), i


@pytest.mark.parametrize("mode", ["emit", "inplace"])
def test_dump_samples_a_large_batch(mode, tmp_path, monkeypatch):
    """Past DUMP_PACKETS packets the dump is a fixed sample: the same rows every run."""
    wl, ref = golden_io.load("config_b_small")
    v = ref["verdict"].astype(np.uint32)
    rec = records_from_reference(wl.frames, ref["frames"], wl.desc, v)
    cap = wl.n // 3
    monkeypatch.setitem(bench.DUMP_PACKETS, mode, cap)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), 0, mode, wl, v,
                           torch.from_numpy(_compacted(rec, v).reshape(-1)),
                           torch.from_numpy(ref["frames"].copy()))
        runs.append(_load_dir(tmp_path / d))
    a, b = runs
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    pick = a["packets"].astype(np.int64)
    assert len(pick) == cap == len(np.unique(pick)) and np.all(np.diff(pick) > 0)
    assert np.array_equal(a["verdict"].astype(np.uint32), v[pick])
    if mode == "emit":
        assert np.array_equal(a["records"].astype("<u4").view(np.uint8).reshape(-1, 16), rec[pick])
    else:
        assert a["frames"].shape == (cap, REWRITE_EXTENT)


def test_dump_sizes_at_the_caps():
    """The caps keep a dump under 64 MB: verdict + packets (8 B each) + the mode's array."""
    assert bench.DUMP_PACKETS["emit"] * (8 + 8 + 4 * 8) <= LIMIT
    assert bench.DUMP_PACKETS["inplace"] * (8 + 8 + REWRITE_EXTENT * 4) <= LIMIT

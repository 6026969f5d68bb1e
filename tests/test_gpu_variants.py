"""GPU: the public kernel-variant word (upe_launch_info_t.variant, include/upe_gpu.h) names the
path a launch took: neither bit 4 (ring) nor bit 5 (host path) for a device batch, both for the
egress-list kernels, bit 5 alone for mapped host memory; bit 0 says emit mode.  (Ring launches:
tests/test_gpu_ring.py.)"""
from __future__ import annotations

import numpy as np
import pytest

import golden_io
from upe_amd import gpu

pytestmark = pytest.mark.gpu

VAR_EMIT = 1   # bit 0 of the variant word


def test_variant_word_names_the_path(gpu_worker_factory):
    wl, _ = golden_io.load("config_b_small")
    n = wl.n
    w = gpu_worker_factory(wl.capacity)
    pf = gpu.PinnedArray(wl.frames.shape, np.uint8)
    pd = gpu.PinnedArray(wl.desc.shape, np.uint64)
    pv = gpu.PinnedArray((n,), np.uint32)
    got = []
    try:
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        tx = w.malloc(4 * n)
        cnt = w.malloc(4 * ((n + 63) // 64))
        b.run()                                                          # in place
        got.append(w.launch_info()["variant"])
        b.run_emit()                                                     # emit
        got.append(w.launch_info()["variant"])
        w.process_emit_tx(b.frames, b.desc, b.verdict, b.hdr, tx, cnt, n)   # emit + egress list
        got.append(w.launch_info()["variant"])
        pf.array[:] = wl.frames
        pd.array[:] = wl.desc
        w.process_mapped(pf.array, pd.array, pv.array)                   # mapped host memory
        got.append(w.launch_info()["variant"])
        w.sync()
        w.free(tx)
        w.free(cnt)
        b.free()
    finally:
        w.close()
        for p in (pf, pd, pv):
            p.free()
    path = gpu.VAR_RING | gpu.VAR_HOST
    assert [v & path for v in got] == [0, 0, 48, 32], got
    assert [bool(v & VAR_EMIT) for v in got] == [False, True, True, False], got

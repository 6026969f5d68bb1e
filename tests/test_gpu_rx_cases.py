"""GPU: upe_gpu_rx_dispatch on the chosen batches of tests/rx_cases.py (pinned without a GPU by
tests/test_rx_cases.py), bit for bit against rx.dispatch_host over the pool's reference hashes:
every ring count from 1 to 64, every pattern at the sizes around a wave, a workgroup, a tile and
nine tiles, and four patterns at the sizes around the scan's step of 512 tiles; a context's scratch
reused after a larger batch and another ring count; two calls queued on a caller's stream; the
optional outputs left out.  Every output has room for GUARD elements more than n, poisoned like
the rest, and they must hold the poison after the call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rx_cases as rc
from test_gpu_keys import dev_in
from test_gpu_latency import _hip
from test_gpu_rx_dispatch import _check
from upe_amd import rx

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 16
FIELDS = (("ring", np.uint32), ("index", np.uint32), ("flow_hash", np.uint32),
          ("desc_out", np.uint64))


class Outs:
    """The device outputs of a context's dispatches of up to cap packets, allocated once: arm()
    poisons what a call of n packets may write and GUARD elements behind it, fetch() reads both
    back and wants the poison behind."""

    def __init__(self, w, cap, flow_hash=True, desc_out=True):
        self.w = w
        self.ptr = {k: w.malloc(np.dtype(t).itemsize * (cap + GUARD)) for k, t in FIELDS
                    if {"flow_hash": flow_hash, "desc_out": desc_out}.get(k, True)}
        self.ptr["counts"] = w.malloc(8 * (rc.RING_IDS + 1 + GUARD))
        self.poison = np.full(8 * (max(cap, rc.RING_IDS + 1) + GUARD), POISON, np.uint8)

    def _sizes(self, n, rings):
        for k, t in FIELDS + (("counts", np.uint64),):
            if k in self.ptr:
                yield k, np.dtype(t), (rings + 1 if k == "counts" else n) + GUARD

    def arm(self, n, rings):
        for k, t, m in self._sizes(n, rings):
            self.w.h2d(self.ptr[k], self.poison[:t.itemsize * m])
        self.w.sync()

    def call(self, frames, desc, n, rings, rr, stream=None):
        p = self.ptr
        self.w.rx_dispatch(frames, desc, n, rings, rr, p["ring"], p["index"], p["counts"],
                           flow_hash=p.get("flow_hash"), desc_out=p.get("desc_out"), stream=stream)

    def fetch(self, n, rings, what=""):
        self.w.sync()
        got = {}
        for k, t, m in self._sizes(n, rings):
            got[k] = np.empty(m, t)
            self.w.d2h(got[k], self.ptr[k])
        self.w.sync()
        for k, a in got.items():
            assert (a[-GUARD:].view(np.uint8) == POISON).all(), f"{what}: {k} written past its end"
            got[k] = a[:-GUARD]
        return got

    def free(self):
        for p in self.ptr.values():
            self.w.free(p)


class Bench:
    """One context with the pool uploaded once, a descriptor buffer and the outputs."""

    def __init__(self, factory, cap, **kw):
        self.w = factory(16)
        self.frames = dev_in(self.w, rc.pool()[0])
        self.desc = self.w.malloc(8 * cap)
        self.out = Outs(self.w, cap, **kw)

    def run(self, desc, rings, rr, what):
        n = len(desc)
        self.w.h2d(self.desc, desc)
        self.out.arm(n, rings)
        self.out.call(self.frames, self.desc, n, rings, rr)
        return self.out.fetch(n, rings, what)

    def close(self):
        self.out.free()
        self.w.free(self.desc)
        self.w.free(self.frames)
        self.w.close()


def _closed(got, n, rings, pattern, rr, what):
    """The three patterns whose dispatch is written out by hand, against that."""
    if pattern in rc.CLOSED:
        ring, index, counts = rc.closed_form(n, rings, pattern, rr)
        assert np.array_equal(got["ring"], ring), f"{what}: closed form, ring"
        assert np.array_equal(got["index"], index), f"{what}: closed form, index"
        assert np.array_equal(got["counts"], counts), f"{what}: closed form, counts"


@pytest.mark.parametrize("rings", rc.RINGS)
def test_small_sweep(gpu_worker_factory, rings):
    b = Bench(gpu_worker_factory, max(rc.SMALL))
    try:
        for pattern in rc.PATTERNS:
            for n in rc.SMALL:
                desc, hashes, ok = rc.batch(n, rings, pattern)
                for rr in (0, rings - 1, 0x7FFFFFF3):
                    what = f"{pattern} n {n} rings {rings} rr {rr:#x}"
                    got = b.run(desc, rings, rr, what)
                    _check(got, hashes, ok, desc, rings, rr, what)
                    _closed(got, n, rings, pattern, rr & (rings - 1), what)
    finally:
        b.close()


@pytest.mark.parametrize("rings", rc.RINGS)
def test_large(gpu_worker_factory, rings):
    """Around the scan's step: a second and a third iteration of its loop, its carries, and
    every lane of its wave prefix."""
    b = Bench(gpu_worker_factory, max(rc.LARGE))
    rr = rings - 1
    try:
        for pattern in rc.LARGE_PATTERNS:
            for n in rc.LARGE:
                desc, hashes, ok = rc.batch(n, rings, pattern)
                what = f"{pattern} n {n} rings {rings}"
                got = b.run(desc, rings, rr, what)
                _check(got, hashes, ok, desc, rings, rr, what)
                _closed(got, n, rings, pattern, rr, what)
    finally:
        b.close()


def test_stale_scratch(gpu_worker_factory):
    """The scratch table's layout follows the tile count and the ring count, and a context keeps
    it between calls: a large batch at 64 rings, then every small case at 8 rings from the
    largest down, then at 32 rings from the smallest up, every call checked; then all of it once
    more, and each call's bytes are those of its first run."""
    big = 520 * 1024 + 5
    assert big in rc.LARGE
    plan = [("seeded", big, 64)]
    plan += [(p, n, 8) for n in sorted(rc.SMALL, reverse=True) for p in rc.PATTERNS]
    plan += [(p, n, 32) for n in sorted(rc.SMALL) for p in rc.PATTERNS]
    b = Bench(gpu_worker_factory, big)
    first = {}
    try:
        for again in (False, True):
            for pattern, n, rings in plan:
                desc, hashes, ok = rc.batch(n, rings, pattern)
                what = f"{pattern} n {n} rings {rings}" + (", second run" if again else "")
                got = b.run(desc, rings, rings - 1, what)
                if not again:
                    _check(got, hashes, ok, desc, rings, rings - 1, what)
                    first[pattern, n, rings] = got
                    continue
                for k, a in first[pattern, n, rings].items():
                    assert a.tobytes() == got[k].tobytes(), f"{what}: {k} differs from the first"
    finally:
        b.close()


def test_callers_stream(gpu_worker_factory):
    """Two dispatches of different n and rings queued back to back on a stream of the caller's,
    nothing waited for in between (the second needs more scratch than the first left): each
    output holds its own call's result."""
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    calls = (("runs", 8193, 16, 15), ("seeded", 520 * 1024 + 5, 32, 7))
    w = gpu_worker_factory(16)
    try:
        frames = dev_in(w, rc.pool()[0])
        batches = [rc.batch(n, rings, p) for p, n, rings, _ in calls]
        descs = [dev_in(w, x[0]) for x in batches]
        outs = [Outs(w, n) for _, n, _, _ in calls]
        for o, (_, n, rings, _) in zip(outs, calls):
            o.arm(n, rings)
        for o, d, (_, n, rings, rr) in zip(outs, descs, calls):
            o.call(frames, d, n, rings, rr, stream=s.value)
        w.sync(s.value)
        for o, (desc, hashes, ok), (p, n, rings, rr) in zip(outs, batches, calls):
            what = f"{p} n {n} rings {rings} on a caller's stream"
            _check(o.fetch(n, rings, what), hashes, ok, desc, rings, rr, what)
            o.free()
        for d in descs + [frames]:
            w.free(d)
    finally:
        w.close()
        assert hip.hipStreamDestroy(s) == 0


def test_optional_outputs_absent(gpu_worker_factory):
    """d_flow_hash and d_desc_out NULL at 513 tiles and 16 rings: ring, index and counts as with
    them."""
    n, rings, rr = 512 * 1024 + 1, 16, 15
    assert n in rc.LARGE and -(-n // rc.BLOCK) == rc.SCAN_STEP + 1
    desc, hashes, ok = rc.batch(n, rings, "seeded")
    ring, index, counts, _ = rx.dispatch_host(hashes, ok, rings, rr)
    b = Bench(gpu_worker_factory, n, flow_hash=False, desc_out=False)
    try:
        got = b.run(desc, rings, rr, "optional outputs absent")
    finally:
        b.close()
    assert set(got) == {"ring", "index", "counts"}
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["ring"], ring) and np.array_equal(got["index"], index)

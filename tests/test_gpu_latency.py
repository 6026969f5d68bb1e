"""GPU: upe_gpu_latency_record, the worker's per-packet latency histogram accumulated on the
device from a batch's timestamps and verdict words.  Expected values come from
latency.record_host, which tests/test_latency_cases.py pins to the reference's latency_record;
every comparison is of all 12 histogram words, bit for bit."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import golden_io
import latency_cases
import oracle
from upe_amd import gpu, ingress, latency
from upe_amd.layout import HDR_WINDOW, V_CONSUMED, desc_lens, desc_offsets

pytestmark = pytest.mark.gpu

B = gpu.LATENCY_BLOCK   # packets per workgroup pass of the kernel
CASES = latency_cases.cases()
# (66 B + 3: more workgroups than the device keeps copies of the histogram)
SIZES = [1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 17, 66 * B + 3]
INIT = latency.init().tolist()


@pytest.fixture(scope="module")
def worker(gpu_worker_factory):
    w = gpu_worker_factory(64)
    yield w
    w.close()


def _upload(w, a, stream=None):
    a = np.ascontiguousarray(a)
    p = w.malloc(max(a.nbytes, 16))
    if a.nbytes:
        w.h2d(p, a, stream)
    if stream is None:
        w.sync()
    return p


def _record(w, c, stream=None):
    """One case through the device call, with the case's calibration."""
    d_ts = _upload(w, c.ts, stream)
    d_v = _upload(w, c.verdicts, stream) if c.verdicts is not None else 0
    try:
        w.set_tsc(c.cpn)
        w.latency_record(d_ts, d_v or None, len(c.ts), c.now, stream)
        return w.get_latency()
    finally:
        w.free(d_ts)
        if d_v:
            w.free(d_v)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_cases(worker, c):
    worker.reset_latency()
    assert _record(worker, c).tolist() == latency_cases.expected(c).tolist()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(worker, n):
    c = latency_cases.sized(n)
    worker.reset_latency()
    assert _record(worker, c).tolist() == latency_cases.expected(c).tolist()
    worker.reset_latency()
    assert _record(worker, c._replace(verdicts=None)).tolist() == \
        latency_cases.expected(c._replace(verdicts=None)).tolist()


@pytest.mark.parametrize("cap", ["1", "8"])
def test_grid_stride_later_passes(gpu_worker_factory, monkeypatch, cap):
    """UPE_GPU_GRID_CAP workgroups at most: with 8, workgroups 0..2 of a 10 B + 77 packet batch
    make a second pass (the last one a partial tile); with 1, one workgroup makes all eleven."""
    monkeypatch.setenv("UPE_GPU_GRID_CAP", cap)
    w = gpu_worker_factory(64)
    try:
        for n in (8 * B, 8 * B + 1, 10 * B + 77):
            c = latency_cases.sized(n)
            w.reset_latency()
            assert _record(w, c).tolist() == latency_cases.expected(c).tolist(), n
    finally:
        w.close()


def test_accumulates_over_calls_and_calibrations(worker):
    """Three calls with their own `now`, the calibration changed in between: the histogram is the
    mirror's after the same three batches, at every step."""
    worker.reset_latency()
    want = latency.init()
    steps = [latency_cases.sized(B + 5, 1, 2.4), latency_cases.sized(700, 2, 0.7)._replace(now=2**62),
             latency_cases.sized(2 * B + 1, 3, 3.3333333333)._replace(now=12345)]
    for c in steps:
        want = latency_cases.expected(c, start=want)
        assert _record(worker, c).tolist() == want.tolist(), c.name
    assert int(want[latency.TOTAL]) > 2000


def test_reset_latency(worker):
    c = latency_cases.sized(300)
    worker.reset_latency()
    assert _record(worker, c).tolist() != INIT
    worker.reset_latency()
    assert worker.get_latency().tolist() == INIT
    assert _record(worker, c).tolist() == latency_cases.expected(c).tolist()


def test_other_resets_and_loads_leave_it_alone(gpu_worker_factory):
    """upe_gpu_reset_stats, a rule reload, upe_gpu_load_rules and upe_gpu_load_neigh do not touch
    the histogram (the reference keeps latency_hist across a SIGHUP), nor does a classify launch;
    it goes on accumulating afterwards."""
    wl, _ = golden_io.load("config_b_small")
    c = latency_cases.sized(B + 9)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        want = latency_cases.expected(c)
        assert _record(w, c).tolist() == want.tolist()
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.run()
        b.fetch()
        assert w.get_latency().tolist() == want.tolist(), "a classify launch"
        w.reset_stats()
        assert w.get_latency().tolist() == want.tolist(), "reset_stats"
        w.reload_rules(wl.rules_sorted[: len(wl.rules_sorted) // 2], capacity=2 * wl.capacity)
        assert w.get_latency().tolist() == want.tolist(), "reload_rules"
        w.reload_image(gpu.RuleImage(wl.rules_sorted, wl.capacity))
        assert w.get_latency().tolist() == want.tolist(), "reload_image"
        w.load_rules(wl.rules_sorted)
        assert w.get_latency().tolist() == want.tolist(), "load_rules"
        w.load_neigh(wl.arp, wl.ndp)
        w.load_neigh(None, None)
        assert w.get_latency().tolist() == want.tolist(), "load_neigh"
        b.run_emit()
        b.fetch()
        b.free()
        want = latency_cases.expected(c, start=want)
        assert _record(w, c).tolist() == want.tolist(), "accumulating afterwards"
    finally:
        w.close()


def _hip():
    """The HIP runtime the library is linked against (already loaded with it)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("libupe_gpu.so loaded no libamdhip64.so")


def test_callers_stream(worker):
    """Uploads and the call queued on a stream of the caller's, nothing waited for in between."""
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        worker.reset_latency()
        want = latency.init()
        for c in (latency_cases.sized(3 * B + 17, 4), latency_cases.sized(65, 5)):
            want = latency_cases.expected(c, start=want)
            assert _record(worker, c, stream=s.value).tolist() == want.tolist()
    finally:
        worker.sync(s.value)
        assert hip.hipStreamDestroy(s) == 0


def test_errors_change_nothing(gpu_worker_factory):
    """-1 with a message and no launch: no calibration yet, a refused calibration, NULL arguments,
    n beyond 32 bits.  n == 0 succeeds and launches nothing.  The histogram is the same after
    each, and a valid call afterwards passes."""
    c = latency_cases.sized(B + 1)
    w = gpu_worker_factory(64)
    L = gpu.LIB
    try:
        d_ts, d_v = _upload(w, c.ts), _upload(w, c.verdicts)
        n = len(c.ts)
        with pytest.raises(gpu.UpeGpuError, match="calibration"):
            w.latency_record(d_ts, d_v, n, c.now)
        with pytest.raises(gpu.UpeGpuError, match="calibration"):
            w.latency_record(d_ts, d_v, 0, c.now)
        assert w.get_latency().tolist() == INIT
        for bad in (0.0, -2.4, float("nan"), float("inf")):
            with pytest.raises(gpu.UpeGpuError, match="cycles_per_ns"):
                w.set_tsc(bad)
        with pytest.raises(gpu.UpeGpuError, match="calibration"):   # none of them took
            w.latency_record(d_ts, d_v, n, c.now)
        assert L.upe_gpu_set_tsc(None, 2.4) == -1
        w.set_tsc(c.cpn)
        w.latency_record(d_ts, d_v, n, c.now)
        want = latency_cases.expected(c)
        assert w.get_latency().tolist() == want.tolist()
        for bad in (0.0, float("nan")):                              # the calibration stays
            with pytest.raises(gpu.UpeGpuError):
                w.set_tsc(bad)
        assert L.upe_gpu_latency_record(None, d_ts, d_v, n, c.now, None) == -1
        assert L.upe_gpu_latency_record(w._ctx, None, d_v, n, c.now, None) == -1
        assert L.upe_gpu_latency_record(w._ctx, d_ts, d_v, 2**32 - B, c.now, None) == -1
        assert L.upe_gpu_latency_record(w._ctx, d_ts, d_v, 2**40, c.now, None) == -1
        assert L.upe_gpu_last_error()
        assert L.upe_gpu_get_latency(None, None) == -1
        assert L.upe_gpu_get_latency(w._ctx, None) == -1
        assert L.upe_gpu_reset_latency(None) == -1
        assert w.get_latency().tolist() == want.tolist()
        w.latency_record(d_ts, d_v, 0, c.now)                        # nothing to do
        w.latency_record(None, None, 0, c.now)
        assert w.get_latency().tolist() == want.tolist()
        w.latency_record(d_ts, d_v, n, c.now)
        assert w.get_latency().tolist() == latency_cases.expected(c, start=want).tolist()
        w.free(d_ts)
        w.free(d_v)
    finally:
        w.close()


def test_gather_classify_record(gpu_worker_factory):
    """The resident pipeline: a pool whose buffers carry timestamps (some zero, one later than
    `now`) and frames of every exit of process_packet — NS/NA that are consumed and ARP among
    them — through upe_gpu_ingress_gather (WINDOW), upe_gpu_process_emit and
    upe_gpu_latency_record with the gather's own d_timestamp.  The histogram is the mirror's over
    the pool's timestamps and the restated worker's verdicts."""
    wl, _ = golden_io.load("edge_zero")
    ref = oracle.run_restated(wl, apply_control=False)
    n = wl.n
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    frames = [wl.frames[o:o + ln] for o, ln in zip(offs, lens)]
    rng = np.random.default_rng(99)
    slots = rng.permutation(2 * n)[:n].astype(np.uint32)
    now, cpn = 1 << 41, 2.4
    ts = np.uint64(now) - latency_cases.random_cycles(n, 17)
    ts[rng.integers(0, 6, n) == 0] = 0
    ts[7] = now + 1000                                   # stamped after `now`: the cycles wrap
    consumed = (ref.verdict & 0xF) == V_CONSUMED
    assert consumed.sum() >= 4 and np.count_nonzero(ts[consumed]) >= 2
    pool = ingress.make_pool(frames, lens, slots, 2 * n, 2064, timestamps=ts)
    want = latency.record_host(latency.init(), ts, ref.verdict, now, cpn)
    assert int(want[latency.TOTAL]) < int(latency.record_host(latency.init(), ts, None, now,
                                                              cpn)[latency.TOTAL])
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        w.set_tsc(cpn)
        d_pool, d_slot = _upload(w, pool), _upload(w, slots)
        d_out = _upload(w, np.zeros(n * HDR_WINDOW + 96, np.uint8))
        d_desc, d_ts, d_info = w.malloc(8 * n), w.malloc(8 * n), w.malloc(64)
        d_verdict, d_hdr = w.malloc(4 * n), w.malloc(16 * n)
        w.ingress_gather(d_pool, pool.size, 2064, d_slot, n, ingress.WINDOW, d_desc, d_info,
                         out=d_out, out_bytes=n * HDR_WINDOW, timestamp=d_ts)
        w.process_emit(d_out, d_desc, d_verdict, d_hdr, n)
        w.latency_record(d_ts, d_verdict, n, now)
        got = w.get_latency()
        verdict, back = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        w.d2h(verdict, d_verdict)
        w.d2h(back, d_ts)
        w.sync()
        for p in (d_pool, d_slot, d_out, d_desc, d_ts, d_info, d_verdict, d_hdr):
            w.free(p)
    finally:
        w.close()
    assert np.array_equal(back, ts), "the gather's timestamps"
    assert np.array_equal(verdict & ~np.uint32(0x80), ref.verdict & ~np.uint32(0x80))
    assert got.tolist() == want.tolist()

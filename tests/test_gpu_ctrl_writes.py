"""upe_gpu_ctrl_writes on the device against its numpy twin (upe_amd/ctrl.py, pinned to the
reference's tables and to hand-written expectations by tests/test_ctrl_writes.py), byte for byte:
every batch of tests/ctrl_cases.py at five capacities, the goldens through upe_neigh_apply_writes,
upe_gpu_process_segmented's tables, a caller's stream, offsets past 4 GiB, the error matrix.  The
record buffer is poisoned before every call and followed by a canary (tests/test_gpu_keys.py's
Out)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import ctrl_cases as cc
import golden_io
from test_ctrl_writes import GOLDENS, KEEP, NOW, raw
from test_gpu_keys import POISON, Out, dev_in
from test_gpu_latency import _hip
from upe_amd import ctrl, gpu
from upe_amd.layout import CTRL_INFO_DTYPE, CTRL_WRITE_DTYPE

pytestmark = pytest.mark.gpu


def caps_of(writes: int):
    return sorted({c for c in (0, 1, writes - 1, writes, writes + 7) if c >= 0})


def device_call(w, df, dd, n, cap, stream=None):
    """One call into poisoned outputs: (the record buffer's cap * 32 bytes, the info's 32)."""
    out, info = Out(w, 32 * cap), Out(w, 32)
    w.ctrl_writes(df, dd, n, out.ptr, cap, info.ptr, stream=stream)
    if stream:
        w.sync(stream)
    return out.fetch(), info.fetch()


def check(w, frames, desc, what, caps=None, stream=None):
    """The device's bytes against the twin's at every cap; returns all the records."""
    want, winfo = ctrl.ctrl_writes(frames, desc)
    df, dd = dev_in(w, frames), dev_in(w, desc)
    for cap in caps_of(len(want)) if caps is None else caps:
        got, ginfo = device_call(w, df, dd, len(desc), cap, stream)
        stored = min(cap, len(want))
        winfo["stored"] = stored
        assert ginfo.tobytes() == raw(winfo), (what, cap, ginfo.view(np.uint64), winfo)
        assert got[:32 * stored].tobytes() == raw(want[:stored]), (what, cap)
        assert (got[32 * stored:] == POISON).all(), f"{what}: a slot from `stored` on was written"
    w.free(df)
    w.free(dd)
    return want


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
def test_chosen_frames(gpu_worker_factory, poison):
    frames, desc = cc.chosen_batch(poison)
    with gpu_worker_factory(16) as w:
        want = check(w, frames, desc, "chosen")
    assert len(want) > 20 and raw(want) == raw(ctrl.ctrl_writes(*cc.chosen_batch())[0])


@pytest.mark.parametrize("n", cc.SIZES)
def test_placement(gpu_worker_factory, n):
    with gpu_worker_factory(16) as w:
        for p in cc.PATTERNS:
            frames, desc, pos = cc.placement(n, p)
            want = check(w, frames, desc, f"{p} n={n}")
            assert np.array_equal(want["index"], pos)


def device_records(w, frames, desc, stream=None):
    want, _ = ctrl.ctrl_writes(frames, desc)
    df, dd = dev_in(w, frames), dev_in(w, desc)
    got, info = device_call(w, df, dd, len(desc), len(want) + 3, stream)
    w.free(df)
    w.free(dd)
    info = info.view(CTRL_INFO_DTYPE)[0]
    assert info["writes"] == info["stored"] == len(want)
    return got[:32 * len(want)].view(CTRL_WRITE_DTYPE).copy()


@pytest.mark.parametrize("case", GOLDENS)
def test_goldens_reference_tables(gpu_worker_factory, case):
    wl, ref = golden_io.load(case)
    with gpu_worker_factory(wl.capacity) as w:
        writes = device_records(w, wl.frames, wl.desc)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    assert gpu.neigh_apply_writes(arp, ndp, writes, NOW) == len(writes)
    assert np.array_equal(arp[KEEP], ref["arp"][KEEP])
    assert np.array_equal(ndp[KEEP], ref["ndp"][KEEP])


def test_against_process_segmented(gpu_worker_factory):
    wl, _ = golden_io.load("ndp_walk")
    with gpu_worker_factory(wl.capacity) as w:
        writes = device_records(w, wl.frames, wl.desc)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    applied = gpu.neigh_apply_writes(arp, ndp, writes, NOW)
    sarp, sndp = wl.arp.copy(), wl.ndp.copy()
    with gpu_worker_factory(wl.capacity) as w2:
        w2.configure(wl)
        b = gpu.DeviceBatch(w2, wl.frames, wl.desc)
        n_writes = w2.process_segmented(b.frames, b.desc, b.verdict, b.n, sarp, sndp, now=NOW)
        b.free()
    assert applied == n_writes > 0
    assert raw(arp) == raw(sarp) and raw(ndp) == raw(sndp)


def test_callers_stream(gpu_worker_factory):
    """The same on a stream of the caller's; two calls queued back to back on one context, nothing
    waited for in between: each output holds its own call's records, the scratch the second's."""
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    a = cc.placement(2049, "mix")[:2]
    b = cc.chosen_batch()
    try:
        with gpu_worker_factory(16) as w:
            check(w, *b, "chosen on a caller's stream", stream=s.value)
            wants = [ctrl.ctrl_writes(*x) for x in (a, b)]
            devs = [(dev_in(w, x[0]), dev_in(w, x[1]), len(x[1])) for x in (a, b)]
            outs = [(Out(w, 32 * (len(wr) + 2)), Out(w, 32)) for wr, _ in wants]
            for (df, dd, n), (o, i), (wr, _) in zip(devs, outs, wants):
                w.ctrl_writes(df, dd, n, o.ptr, len(wr) + 2, i.ptr, stream=s.value)
            w.sync(s.value)
            for (o, i), (wr, info), name in zip(outs, wants, ("first", "second")):
                got, ginfo = o.fetch(), i.fetch()
                assert ginfo.tobytes() == raw(info), name
                assert got[:32 * len(wr)].tobytes() == raw(wr), name
                assert (got[32 * len(wr):] == POISON).all(), name
            for df, dd, _ in devs:
                w.free(df)
                w.free(dd)
    finally:
        assert hip.hipStreamDestroy(s) == 0


def test_context_untouched(gpu_worker_factory):
    wl, _ = golden_io.load("config_c_small")
    frames, desc = cc.chosen_batch()

    def state(w):
        c, s = w.get_stats()
        return (c.tobytes(), s.tobytes(), w.get_l1().tobytes(), w.get_latency().tobytes(),
                w.launch_info())

    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        w.set_tsc(2.4)
        first = gpu.run_workload(wl, worker=w)
        before = state(w)
        assert before[4]["launches"] == 1
        check(w, frames, desc, "after a classify launch")
        assert state(w) == before
        # and the tables the context classifies with are the ones it had
        w.reset_stats()
        w.set_l1(wl.l1)
        again = gpu.run_workload(wl, worker=w)
        for x, y in zip(first, again):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_offsets_past_4gib(gpu_worker_factory):
    """One allocation of 4 GiB + 64 KiB in device memory, not filled: six control frames at its
    top, the descriptors' offsets on both sides of 2^32."""
    total = (1 << 32) + (64 << 10)
    items = cc.top_six()
    mini, desc = cc.pack(items)
    assert mini.size < 60 << 10
    base = (1 << 32) - 512          # 16-byte aligned; the first frames below 2^32, the rest above
    offs = (desc >> np.uint64(16)) + np.uint64(base)
    assert offs.min() < 1 << 32 < offs.max() and int(offs.max()) + 2048 + 96 <= total
    far = (offs << np.uint64(16)) | (desc & np.uint64(0xFFFF))
    want, winfo = ctrl.ctrl_writes(mini, desc)
    assert len(want) == 5 and winfo["ctrl"] == 6
    with gpu_worker_factory(16) as w:
        big = w.malloc(total)
        w.h2d(big + base, mini)
        dd = dev_in(w, far)
        got, ginfo = device_call(w, big, dd, 6, 6)
        w.free(dd)
        w.free(big)
    assert ginfo.tobytes() == raw(winfo)
    assert got[:32 * 5].tobytes() == raw(want)
    assert (got[32 * 5:] == POISON).all()


def test_error_matrix(gpu_worker_factory):
    L = gpu.LIB
    frames, desc = cc.chosen_batch()
    with gpu_worker_factory(16) as w:
        c = w._ctx
        df, dd = dev_in(w, frames), dev_in(w, desc)
        n = len(desc)
        out, info = Out(w, 32 * 8), Out(w, 32)
        before = w.launch_info()
        O, I = out.ptr, info.ptr
        for args, msg in (((None, df, dd, n, O, 8, I, None), b"null context"),
                          ((c, None, dd, n, O, 8, I, None), b"null buffer"),
                          ((c, df, None, n, O, 8, I, None), b"null buffer"),
                          ((c, df, dd, n, O, 8, None, None), b"null buffer"),
                          ((c, df, dd, n, None, 8, I, None), b"null buffer"),
                          ((c, df, dd, n, O + 8, 7, I, None), b"16-byte aligned"),
                          ((c, df, dd, (1 << 32) - 1024, O, 8, I, None), b"32 bits")):
            assert L.upe_gpu_ctrl_writes(*args) == -1, msg
            assert msg in L.upe_gpu_last_error()
        w.sync()
        assert w.launch_info() == before
        assert (out.fetch() == POISON).all() and (info.fetch() == POISON).all()
        # n == 0: the info zeroed, whatever the batch buffers; cap 0 takes no record buffer
        info = Out(w, 32)
        assert L.upe_gpu_ctrl_writes(c, None, None, 0, None, 0, info.ptr, None) == 0
        z = info.fetch().view(CTRL_INFO_DTYPE)[0]
        assert (z["ctrl"], z["writes"], z["stored"], z["first_write"]) == (0, 0, 0, ctrl.NONE)
        info = Out(w, 32)
        assert L.upe_gpu_ctrl_writes(c, df, dd, n, None, 0, info.ptr, None) == 0
        want, winfo = ctrl.ctrl_writes(frames, desc, 0)
        assert info.fetch().tobytes() == raw(winfo) and winfo["writes"] > 0
        assert w.launch_info() == before
        w.free(df)
        w.free(dd)

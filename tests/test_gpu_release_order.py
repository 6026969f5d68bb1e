"""upe_gpu_release_order on the device against its numpy twin (upe_amd/release.py, pinned to a
restatement of the reference's worker_main by tests/test_release_cases.py), bit for bit: every
case of tests/release_cases.py, handles that repeat and descend and the form without handles, bad
offset arrays, scratch left by a larger batch, a caller's stream, n == 0, the error matrix, and the
handle-in / handle-out chain on the golden configs.  Every output is poisoned before the call and
has 16 poisoned entries of room behind it (and test_gpu_keys.py's canary behind those)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import golden_io
import release_cases as rc
from test_gpu_keys import POISON, Out, dev_in
from test_gpu_latency import _hip
from upe_amd import gpu, ingress, release
from upe_amd.layout import RELEASE_INFO_DTYPE, V_FWD, desc_lens, desc_offsets

pytestmark = pytest.mark.gpu

ROOM = 16
P32 = np.uint32(POISON * 0x01010101)


def device_call(w, verdict, first=None, burst=0, slot=None, want_reply=True, stream=None,
                nb=None):
    """One call into poisoned outputs: (order, handle, burst_fwd, reply, info bytes), each array
    whole — its entries and ROOM more; handle and reply are None where not asked for."""
    n = len(verdict)
    if first is not None and nb is None:
        nb = len(first) - 1
    bursts = nb if first is not None else (n + burst - 1) // burst if burst else 0
    dv = dev_in(w, np.ascontiguousarray(verdict, np.uint32))
    df = dev_in(w, np.ascontiguousarray(first, np.uint32)) if first is not None else 0
    ds = dev_in(w, np.ascontiguousarray(slot, np.uint32)) if slot is not None else 0
    order, bf, info = Out(w, 4 * (n + ROOM)), Out(w, 4 * (bursts + ROOM)), Out(w, 64)
    handle = Out(w, 4 * (n + ROOM)) if slot is not None else None
    reply = Out(w, 4 * (n + ROOM)) if want_reply else None
    w.release_order(dv, n, order.ptr, bf.ptr, info.ptr, first=df or None, nb=nb or 0, burst=burst,
                    slot=ds or None, handle=handle.ptr if handle else None,
                    reply=reply.ptr if reply else None, stream=stream)
    if stream:
        w.sync(stream)
    got = tuple(None if o is None else o.fetch().view(np.uint32)
                for o in (order, handle, bf, reply))
    raw = info.fetch()
    for p in (dv, df, ds):
        if p:
            w.free(p)
    return got + (raw,)


def check(w, verdict, form, slot=None, what="", **kw):
    """The device's outputs against the twin's, poison where the twin writes nothing."""
    exp = release.order_host(verdict, slot=slot, **form)
    order, handle, bf, reply, raw = device_call(w, verdict, slot=slot, **form, **kw)
    assert raw.tobytes() == exp.info.tobytes(), (what, raw.view(np.uint64), exp.info)
    n = len(verdict)
    pairs = [("order", order, exp.order, n), ("burst_fwd", bf, exp.burst_fwd, len(bf) - ROOM),
             ("reply", reply, exp.reply, n)]
    if slot is not None:
        pairs.append(("handle", handle, exp.handle, n))
    for name, got, want, size in pairs:
        if got is None:
            continue
        assert len(got) == size + ROOM
        k = 0 if want is None else len(want)
        assert k == size or name == "reply" or want is None, (what, name)
        assert got[:k].tolist() == ([] if want is None else want.tolist()), (what, name)
        assert (got[k:] == P32).all(), f"{what}: {name} written from entry {k} on"
    return exp


@pytest.mark.parametrize("n", rc.SIZES)
def test_every_case(gpu_worker_factory, n):
    with gpu_worker_factory(16) as w:
        for k, case in enumerate(rc.cases(n)):
            slot = rc.slots(n, ("permuted", "repeat", "descend")[k % 3]) if k % 4 else None
            check(w, case.verdict, case.form, slot, case.name, want_reply=k % 5 != 4)


def test_handles(gpu_worker_factory):
    """Handles that repeat and that descend, and the form without handles, on one batch."""
    n = 2049
    first = rc.SHAPES["cycle"](n)
    v = rc.with_replies(rc.words(rc.fwd_mask(n, 7)), first, "every_burst")
    with gpu_worker_factory(16) as w:
        for kind in ("repeat", "descend", "permuted"):
            for form in ({"first": first}, {"burst": 33}):
                exp = check(w, v, form, rc.slots(n, kind), kind)
                assert exp.handle.tolist() == rc.slots(n, kind)[exp.order].tolist()
        check(w, v, {"first": first}, None, "no handles")
        check(w, v, {"burst": 64}, None, "no handles, no replies", want_reply=False)


@pytest.mark.parametrize("n", (130, 1024, 2049))
def test_bad_burst_arrays(gpu_worker_factory, n):
    v = rc.with_replies(rc.words(rc.fwd_mask(n, 3)), rc.SHAPES["64s"](n), "every_burst")
    with gpu_worker_factory(16) as w:
        good = check(w, v, {"burst": 64}, rc.slots(n, "repeat"), "the valid form first")
        for name, (first, count) in rc.bad_arrays(n).items():
            exp = check(w, v, {"first": first}, rc.slots(n, "repeat"), name)
            assert exp.order is None and int(exp.info["bad_bursts"]) == count, name
            for f in ("forwarded", "consumed", "dropped", "replies", "first_reply"):
                assert exp.info[f] == good.info[f]
        check(w, v, {"first": rc.SHAPES["cycle"](n)}, None, "a valid array after bad ones")


def test_scratch_left_by_a_larger_batch(gpu_worker_factory):
    """One context: a large batch with an offset array, then smaller ones in the other form and
    back — the tile table and the bitmaps of the first call lie behind the later ones'."""
    big, small, mid = 4 * 1024 + 37, 65, 1025
    with gpu_worker_factory(16) as w:
        for n, shape, burst, shift in ((big, "straddle_before", 0, 1), (small, None, 31, 2),
                                       (mid, "cycle", 0, 3), (mid, None, 64, 4),
                                       (small, "ones", 0, 5), (big, None, 48, 6)):
            first = rc.SHAPES[shape](n) if shape else release.fixed_first(n, burst)
            v = rc.with_replies(rc.words(rc.fwd_mask(n, shift)), first, "burst_last")
            form = {"burst": burst} if burst else {"first": first}
            check(w, v, form, rc.slots(n, "permuted"), f"{n}:{shape or burst}")


def test_callers_stream(gpu_worker_factory):
    """On a stream of the caller's; and two calls queued back to back on one context, nothing
    waited for in between: each output holds its own call's lists."""
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        with gpu_worker_factory(16) as w:
            n = 2049
            first = rc.SHAPES["straddle_mid"](n)
            v = rc.with_replies(rc.words(rc.fwd_mask(n, 9)), first, "burst_first")
            check(w, v, {"first": first}, rc.slots(n, "descend"), "caller's stream", stream=s.value)
            jobs = [(v, first, 0), (v[:1025][::-1].copy(), None, 32)]
            outs = []
            for vv, ff, burst in jobs:
                m = len(vv)
                dv = dev_in(w, vv)
                df = dev_in(w, ff) if ff is not None else 0
                nb = len(ff) - 1 if ff is not None else (m + burst - 1) // burst
                o, b = Out(w, 4 * (m + ROOM)), Out(w, 4 * (nb + ROOM))
                r, i = Out(w, 4 * (m + ROOM)), Out(w, 64)
                w.release_order(dv, m, o.ptr, b.ptr, i.ptr, first=df or None, nb=nb if df else 0,
                                burst=burst, reply=r.ptr, stream=s.value)
                outs.append((dv, df, o, b, r, i))
            w.sync(s.value)
            for (vv, ff, burst), (dv, df, o, b, r, i) in zip(jobs, outs):
                form = {"first": ff} if ff is not None else {"burst": burst}
                exp = release.order_host(vv, **form)
                m = len(vv)
                assert i.fetch().tobytes() == exp.info.tobytes()
                assert o.fetch().view(np.uint32)[:m].tolist() == exp.order.tolist()
                got = b.fetch().view(np.uint32)
                assert got[:len(exp.burst_fwd)].tolist() == exp.burst_fwd.tolist()
                got = r.fetch().view(np.uint32)
                assert got[:len(exp.reply)].tolist() == exp.reply.tolist()
                assert (got[len(exp.reply):] == P32).all()
                w.free(dv)
                if df:
                    w.free(df)
    finally:
        assert hip.hipStreamDestroy(s) == 0


def _state(w):
    c, s = w.get_stats()
    return (c.tobytes(), s.tobytes(), w.get_l1().tobytes(), w.get_latency().tobytes(),
            w.launch_info())


def test_empty_batch_and_error_matrix(gpu_worker_factory):
    L = gpu.LIB
    n = 100
    v = rc.words(rc.fwd_mask(n))
    first = rc.SHAPES["cycle"](n)
    nb = len(first) - 1
    with gpu_worker_factory(16) as w:
        c = w._ctx
        before = _state(w)
        dv, df, ds = dev_in(w, v), dev_in(w, first), dev_in(w, rc.slots(n, "repeat"))
        outs = [Out(w, 4 * (n + ROOM)) for _ in range(4)]
        info = Out(w, 64)
        O, H, B, R = (o.ptr for o in outs)
        I = info.ptr
        big = (1 << 32) - 1024
        for args, msg in (
                ((None, dv, n, None, 0, 32, None, O, None, B, R, I, None), b"null context"),
                ((c, dv, n, None, 0, 32, None, O, None, B, R, None, None), b"null buffer"),
                ((c, None, n, None, 0, 32, None, O, None, B, R, I, None), b"null buffer"),
                ((c, dv, n, None, 0, 32, None, None, None, B, R, I, None), b"null buffer"),
                ((c, dv, n, None, 0, 32, None, O, None, None, R, I, None), b"null buffer"),
                ((c, dv, n, None, 0, 32, ds, O, None, B, R, I, None), b"together"),
                ((c, dv, n, None, 0, 32, None, O, H, B, R, I, None), b"together"),
                ((c, dv, n, None, 0, 0, None, O, None, B, R, I, None), b"burst must be"),
                ((c, dv, n, None, 0, 65, None, O, None, B, R, I, None), b"burst must be"),
                ((c, dv, n, df, 0, 0, None, O, None, B, R, I, None), b"offset array"),
                ((c, dv, n, df, n + 1, 0, None, O, None, B, R, I, None), b"offset array"),
                ((c, dv, 0, df, 1, 0, None, O, None, B, R, I, None), b"offset array"),
                ((c, dv, big, None, 0, 32, None, O, None, B, R, I, None), b"32 bits")):
            assert L.upe_gpu_release_order(*args) == -1, msg
            assert msg in L.upe_gpu_last_error(), (msg, L.upe_gpu_last_error())
        w.sync()
        assert _state(w) == before
        for o in outs + [info]:
            assert (o.fetch() == POISON).all()
        # n == 0: the info alone, zero but for first_reply, in either form
        for args in ((c, None, 0, None, 0, 32, None, None, None, None, None),
                     (c, None, 0, df, 0, 0, None, None, None, None, None)):
            info = Out(w, 64)
            assert L.upe_gpu_release_order(*args, info.ptr, None) == 0
            assert info.fetch().view(np.uint64).tolist() == [0, 0, 0, 0, 0, 0, 2**64 - 1, 0]
        # a valid call leaves the context's counters, rule_stats, L1 state, histogram and launch
        # count alone
        check(w, v, {"first": first}, rc.slots(n, "repeat"), "after the refusals")
        assert _state(w) == before
        for p in (dv, df, ds):
            w.free(p)


@pytest.mark.parametrize("case", ["config_a", "config_b_small", "config_c_small",
                                  "config_cf_small", "config_d_small"])
def test_handles_in_handles_out(gpu_worker_factory, case):
    """ingress_gather (REF) -> process_emit_tx -> latency_record -> release_order with the
    gather's handles: the forwarded ranges are the launch's egress list and upe_gpu_compact's,
    release_flush on the fetched lists sends what tx_flush_groups sends, every handle comes back
    exactly once, and the call leaves counters, rule_stats and the histogram as they were."""
    wl, _ = golden_io.load(case)
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    slots = np.random.default_rng(wl.n).permutation(2 * wl.n)[:wl.n].astype(np.uint32)
    pool = ingress.make_pool([wl.frames[o:o + ln] for o, ln in zip(offs, lens)], lens, slots,
                             2 * wl.n, 2064)
    n, burst = wl.n, 32
    groups = (n + 63) // 64
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        w.set_tsc(2.0)
        d_pool, d_slot = dev_in(w, pool), dev_in(w, slots)
        d_desc, d_ginfo, d_ts = w.malloc(8 * n), w.malloc(64), w.malloc(8 * n)
        d_verdict, d_hdr = w.malloc(4 * n), w.malloc(16 * n)
        d_tx, d_cnt = w.malloc(4 * n), w.malloc(4 * groups)
        d_idx, d_k = w.malloc(4 * n), w.malloc(8)
        w.ingress_gather(d_pool, pool.size, 2064, d_slot, n, ingress.REF, d_desc, d_ginfo,
                         timestamp=d_ts)
        w.process_emit_tx(d_pool, d_desc, d_verdict, d_hdr, d_tx, d_cnt, n)
        w.latency_record(d_ts, d_verdict, n, 1 << 40)
        w.compact(d_verdict, n, V_FWD, d_idx, d_k)
        before = _state(w)
        order, handle, bf, reply = (Out(w, 4 * (n + ROOM)) for _ in range(4))
        info = Out(w, 64)
        w.release_order(d_verdict, n, order.ptr, bf.ptr, info.ptr, burst=burst, slot=d_slot,
                        handle=handle.ptr, reply=reply.ptr)
        w.sync()
        assert _state(w) == before
        buf, desc = np.zeros(pool.size, np.uint8), np.zeros(n, np.uint64)
        verdict = np.zeros(n, np.uint32)
        tx, cnt = np.zeros(n, np.uint32), np.zeros(groups, np.uint32)
        flat, k = np.zeros(n, np.uint32), np.zeros(1, np.uint64)
        for h, p in ((buf, d_pool), (desc, d_desc), (verdict, d_verdict), (tx, d_tx), (cnt, d_cnt),
                     (flat, d_idx), (k, d_k)):
            w.d2h(h, p)
        w.sync()
        order, handle, bf, reply = (o.fetch().view(np.uint32) for o in (order, handle, bf, reply))
        info = info.fetch().view(RELEASE_INFO_DTYPE)[0]
        for p in (d_pool, d_slot, d_desc, d_ginfo, d_ts, d_verdict, d_hdr, d_tx, d_cnt, d_idx, d_k):
            w.free(p)
    exp = release.order_host(verdict, burst=burst, slot=slots)
    nb = len(exp.burst_fwd)
    assert info.tobytes() == exp.info.tobytes()
    assert order[:n].tolist() == exp.order.tolist() and (order[n:] == P32).all()
    assert handle[:n].tolist() == exp.handle.tolist() and (handle[n:] == P32).all()
    assert bf[:nb].tolist() == exp.burst_fwd.tolist() and (bf[nb:] == P32).all()
    r = int(info["replies"])
    assert reply[:r].tolist() == exp.reply.tolist() and (reply[r:] == P32).all()
    assert sorted(handle[:n].tolist()) == sorted(slots.tolist())
    ends = np.minimum(burst * (1 + np.arange(nb)), n)
    fwd = np.concatenate([order[e - int(f):e] for e, f in zip(ends, bf[:nb])])
    lst = np.concatenate([tx[64 * g:64 * g + int(cnt[g])] for g in range(groups)])
    assert fwd.tolist() == lst.tolist() == flat[:int(k[0])].tolist()
    assert int(info["forwarded"]) == int(k[0])
    events, f1, d1 = gpu.release_flush(buf, desc, order[:n], bf[:nb], burst=burst,
                                       handle=handle[:n], reply=reply[:r])
    batches, f2, d2 = gpu.tx_flush(buf, desc, None, burst, groups=(tx, cnt))
    sends = [ev for ev in events if ev[0] == "send"]
    assert len(sends) == len(batches) and (f1, d1) == (f2, d2)
    for ev, (idx, data) in zip(sends, batches):
        assert ev[1].tolist() == idx.tolist() and ev[2] == data
    freed = [h for ev in events if ev[0] == "release" for h in ev[1]]
    assert freed == handle[:n].tolist()
    assert [ev[1] for ev in events if ev[0] == "send_one"] == reply[:r].tolist()

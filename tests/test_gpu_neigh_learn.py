"""upe_gpu_neigh_learn on the device against its host twin (upe_neigh_learn_host, pinned to the
contract and to the reference's update by tests/test_neigh_learn.py), bit for bit: every case of
tests/learn_cases.py, what a classify launch queued before and after a learn reads, the L1 entries
a learn must leave alone, owner words and scratch left by other calls, a caller's stream, the
argument checks, and a patch and a load after a learn.  The deferred list is poisoned before the
call; what lies behind the deferred ranks must keep the poison."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import learn_cases as lc
import neigh_cases as nc
import oracle
import patch_cases as pc
import resolve_cases as rc
from test_gpu_keys import POISON, Out, dev_in
from test_gpu_latency import _hip
from test_gpu_neigh_patch import _fetch, _run, gpu_patch
from test_gpu_parity import _force_dst
from test_gpu_resolve import gpu_resolve
from test_neigh_cases import check_against_reference, workload
from upe_amd import gpu
from upe_amd.layout import CW_ARP, CW_NDP, LEARN_INFO_DTYPE

pytestmark = pytest.mark.gpu

ROOM = 16   # entries behind the deferred list that must keep the poison
FIELDS = LEARN_INFO_DTYPE.names


def _info(x):
    return tuple(int(x[f]) for f in FIELDS)


def gpu_learn(w, recs, want_defer=True, stream=None):
    """(the deferred ranks, info) of one upe_gpu_neigh_learn; the records must come back as they
    went in, and nothing past the deferred ranks may be written."""
    n = len(recs)
    raw = np.ascontiguousarray(recs).view(np.uint8).ravel()
    dw = dev_in(w, raw)
    defer, info = Out(w, 4 * (n + ROOM)), Out(w, 64)
    w.neigh_learn(dw, n, defer.ptr if want_defer else None, info.ptr, stream)
    w.sync(stream)
    x = info.fetch().view(LEARN_INFO_DTYPE)[0]
    d = defer.fetch()
    deferred = int(x["deferred"]) if want_defer else 0
    assert (d[4 * deferred:] == POISON).all(), "written past the deferred ranks"
    after = np.empty(max(raw.size, 1), np.uint8)
    if raw.size:
        w.d2h(after[:raw.size], dw)
        w.sync()
        assert np.array_equal(after[:raw.size], raw), "d_writes was written"
    w.free(dw)
    return d[:4 * deferred].view(np.uint32).copy(), x


def check(w, image, recs, keys, what, stream=None):
    """Teach the loaded snapshot and the twin's image (the same state) recs; deferred ranks, info
    and every answer must agree.  The image is left in the state the device is in."""
    defer_h, info_h = gpu.neigh_learn_host(image, recs)
    want = gpu.neigh_image_lookup_host(image, rc.as_keys(keys))
    defer, info = gpu_learn(w, recs, stream=stream)
    assert _info(info) == _info(info_h), what
    assert np.array_equal(defer, defer_h), what
    got = gpu_resolve(w, keys)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} answers differ, first "
                           f"{int(bad[0])}: {int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}")
    return info_h


@pytest.mark.parametrize("name", lc.CASES)
def test_cases(gpu_worker_factory, name):
    c = lc.case(name)
    image, keys = c.image(), lc.keys(c)
    with gpu_worker_factory(16) as w:
        w.load_neigh_image(image)
        before = gpu_resolve(w, keys)
        info = check(w, image, c.recs, keys, name)
        assert _info(info)[1:5] == c.expect
        if c.expect[0] + c.expect[1]:
            assert not np.array_equal(gpu_resolve(w, keys), before), "the learn changed no answer"
        # the same records again find the owner words as the first call left them: every address
        # that went in is a refresh now
        again = check(w, image, c.recs, keys, name + " again")
        assert int(again["inserted"]) == 0
    image.free()


def test_without_a_defer_list(gpu_worker_factory):
    c = lc.case("unreached:embed:hidden")
    image, keys = c.image(), lc.keys(c)
    with gpu_worker_factory(16) as w:
        w.load_neigh_image(image)
        defer, info = gpu_learn(w, c.recs, want_defer=False)
        _, info_h = gpu.neigh_learn_host(image, c.recs)
        assert _info(info) == _info(info_h) and len(defer) == 0 and int(info["deferred"]) > 0
        assert np.array_equal(gpu_resolve(w, keys),
                              gpu.neigh_image_lookup_host(image, rc.as_keys(keys)))
    image.free()


def test_no_snapshot_loaded(gpu_worker_factory):
    """A context that has loaded nothing: no family has an index, every record is deferred."""
    recs = lc.case("one_new:wrap").recs
    with gpu_worker_factory(16) as w:
        defer, info = gpu_learn(w, recs)
    assert _info(info) == (2, 0, 0, 0, 2, 0, 0, 0) and defer.tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------
# what classify sees
# ---------------------------------------------------------------------------------------------

def _taught(name):
    """The case's workload with 200 packets of each family sent to two new addresses, the records
    that teach them (and refresh what the tables hold), and the tables after the records."""
    cs = nc.case(name)
    wl = workload(name).copy()
    a4, a6 = lc.fresh("arp", 900), lc.fresh("ndp", 900)
    _force_dst(wl, 200, a4, np.frombuffer(a6, np.uint8))
    items = [(CW_ARP, a4), (CW_NDP, a6)]
    for fam, kind in (("arp", CW_ARP), ("ndp", CW_NDP)):
        p = nc.Probe(cs.table(fam))
        items += [(kind, k) for k in cs.own(fam) if p.slot(k) >= 0]
    recs = pc.make(items + [(CW_ARP, a4)], salt=0xD3)
    arp2, ndp2 = wl.arp.copy(), wl.ndp.copy()
    assert gpu.neigh_apply_writes(arp2, ndp2, recs, now=5) == len(recs)
    return wl, recs, arp2, ndp2, a4, a6


@pytest.mark.parametrize("emit", [False, True], ids=["in_place", "emit"])
@pytest.mark.parametrize("name", ["wrap", "embed:wrap"], ids=["staged", "memory"])
def test_classify_before_and_after(gpu_worker_factory, name, emit):
    """process, learn, process on one stream with no synchronisation between: the first batch is
    the reference worker's under the old tables, the second under the tables with the new
    neighbours."""
    wl, recs, arp2, ndp2, _, _ = _taught(name)
    r1 = oracle.run_restated(wl)
    wl2 = wl.copy()
    wl2.arp, wl2.ndp, wl2.l1 = arp2, ndp2, r1.l1.copy()
    r2 = oracle.run_restated(wl2)
    check_against_reference(wl2, r2, name + " after the learn")
    old = wl.copy()
    old.l1 = r1.l1.copy()
    assert not np.array_equal(oracle.run_restated(old).frames, r2.frames), "the learn is not seen"
    image = gpu.NeighImage(wl.arp, wl.ndp, room=lc._room(wl.arp))
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        w.load_neigh_image(image)
        b1, b2 = gpu.DeviceBatch(w, wl.frames, wl.desc), gpu.DeviceBatch(w, wl.frames, wl.desc)
        raw = np.ascontiguousarray(recs).view(np.uint8).ravel()
        dw, di = dev_in(w, raw), w.malloc(64)
        _run(b1, emit)
        w.neigh_learn(dw, len(recs), None, di)
        _run(b2, emit)
        f1, v1 = _fetch(b1, wl, emit)
        f2, v2 = _fetch(b2, wl, emit)
        l1 = w.get_l1()
        x = np.zeros(1, LEARN_INFO_DTYPE)
        w.d2h(x.view(np.uint8).ravel(), di)
        w.sync()
        for p in (dw, di):
            w.free(p)
        b1.free(), b2.free()
    image.free()
    assert _info(x[0])[1:5] == (len(recs) - 2, 2, 0, 0)
    assert np.array_equal(v1, r1.verdict) and np.array_equal(f1, r1.frames), "before the learn"
    assert np.array_equal(v2, r2.verdict), "after the learn"
    assert np.array_equal(f2, r2.frames), "after the learn"
    assert l1.tobytes() == r2.l1.tobytes()


@pytest.mark.parametrize("emit", [False, True], ids=["in_place", "emit"])
def test_l1_entries_keep_the_old_mac(gpu_worker_factory, emit):
    """The L1 entries hold the addresses being taught, with other MACs: the reference never
    invalidates them, so packets aimed at an entry go on with the old MAC."""
    name = "wrap"
    wl, recs, arp2, ndp2, a4, a6 = _taught(name)
    l1 = wl.l1.copy()
    l1["last_arp_ip"] = a4
    l1["last_arp_mac"] = np.frombuffer(bytes([2, 0x11, 0x22, 0x33, 0x44, 0x55]), np.uint8)
    l1["last_ndp_ip"] = np.frombuffer(a6, np.uint8)
    l1["last_ndp_mac"] = np.frombuffer(bytes([2, 0x66, 0x77, 0x88, 0x99, 0xAA]), np.uint8)
    wl.l1 = l1
    wl2 = wl.copy()
    wl2.arp, wl2.ndp = arp2, ndp2
    r = oracle.run_restated(wl2)
    check_against_reference(wl2, r, name + " L1")
    image = gpu.NeighImage(wl.arp, wl.ndp, room=(64, 64))
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        w.load_neigh_image(image)
        defer, info = gpu_learn(w, recs)
        assert len(defer) == 0 and int(info["inserted"]) == 2
        assert w.get_l1().tobytes() == l1.tobytes(), "the learn touched the L1 entries"
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        _run(b, emit)
        frames, verdict = _fetch(b, wl, emit)
        b.free()
        assert np.array_equal(verdict, r.verdict)
        assert np.array_equal(frames, r.frames)
        assert w.get_l1().tobytes() == r.l1.tobytes()
    image.free()


# ---------------------------------------------------------------------------------------------
# the context around a learn
# ---------------------------------------------------------------------------------------------

def test_after_a_larger_call_and_a_patch(gpu_worker_factory):
    """Owner words and scratch left by a larger learn and by a patch; then a patch after a learn
    refreshes what the learn put in; then a load supersedes the device state."""
    big, small = lc.case("count:2049"), lc.case("shared_first:")
    with gpu_worker_factory(16) as w:
        image = big.image()
        w.load_neigh_image(image)
        check(w, image, big.recs, lc.keys(big), "the larger call")
        image.free()
        image, keys = small.image(), lc.keys(small)
        w.load_neigh_image(image)
        info = check(w, image, small.recs, keys, "after the larger call")
        assert _info(info)[1:5] == small.expect
        # a patch of the addresses just learnt: all held
        again = pc.make([(int(k), bytes(ip) if k == CW_NDP else
                          int.from_bytes(bytes(ip[:4]), "little"))
                         for k, ip in zip(small.recs["kind"], small.recs["ip"])], salt=0x99)
        miss, pinfo = gpu_patch(w, again)
        miss_h, _ = gpu.neigh_patch_host(image, again)
        assert len(miss) == 0 and len(miss_h) == 0 and int(pinfo["patched"]) == len(again)
        assert np.array_equal(gpu_resolve(w, keys),
                              gpu.neigh_image_lookup_host(image, rc.as_keys(keys)))
        # and a learn after the patch
        check(w, image, small.recs, keys, "after the patch")
        image.free()
        # a load supersedes what was learnt: the free counts and the index are the image's again
        image = small.image()
        w.load_neigh_image(image)
        info = check(w, image, small.recs, keys, "after a load")
        assert _info(info)[1:5] == small.expect
        image.free()


def test_callers_stream(gpu_worker_factory):
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    c = lc.case("interleaved:embed:wrap")
    image, keys = c.image(), lc.keys(c)
    try:
        with gpu_worker_factory(16) as w:
            w.load_neigh_image(image)
            info = check(w, image, c.recs, keys, "a caller's stream", stream=s.value)
            assert _info(info)[1:5] == c.expect
    finally:
        assert hip.hipStreamDestroy(s) == 0
        image.free()


def test_untouched_state(gpu_worker_factory):
    name = "embed:wrap"
    wl = workload(name)
    c = lc.case("interleaved:embed:wrap")
    keys = lc.keys(c)
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        gpu.run_workload(wl, worker=w)
        image = c.image()
        w.load_neigh_image(image)
        old = gpu_resolve(w, keys)

        def state():
            cn, s = w.get_stats()
            return cn.tobytes(), s.tobytes(), w.get_latency().tobytes(), w.launch_info()

        before = state()
        _, info = gpu_learn(w, c.recs)
        assert int(info["inserted"]) > 0
        assert state() == before
        assert not np.array_equal(gpu_resolve(w, keys), old)
        # the image is a value: the dry run still answers as before the learn
        assert np.array_equal(gpu_resolve(w, keys, image=image), old)
        image.free()


def test_argument_errors_and_empty(gpu_worker_factory):
    L = gpu.LIB
    c = lc.case("one_new:wrap")
    image, keys = c.image(), lc.keys(c)
    with gpu_worker_factory(16) as w:
        ctx = w._ctx
        w.load_neigh_image(image)
        old = gpu_resolve(w, keys)
        buf = dev_in(w, np.ascontiguousarray(c.recs).view(np.uint8).ravel())
        defer, info = Out(w, 256), Out(w, 64)
        before = w.launch_info()
        assert L.upe_gpu_neigh_learn(None, buf, 1, defer.ptr, info.ptr, None) == -1
        assert b"null context" in L.upe_gpu_last_error()
        for args in ((ctx, buf, 1, defer.ptr, None, None), (ctx, None, 1, defer.ptr, info.ptr, None)):
            assert L.upe_gpu_neigh_learn(*args) == -1
            assert b"null buffer" in L.upe_gpu_last_error()
        assert L.upe_gpu_neigh_learn(ctx, buf + 8, 1, defer.ptr, info.ptr, None) == -1
        assert b"aligned" in L.upe_gpu_last_error()
        assert L.upe_gpu_neigh_learn(ctx, buf, (1 << 32) - gpu.LEARN_CHUNK, defer.ptr, info.ptr,
                                     None) == -1
        assert b"32 bits" in L.upe_gpu_last_error()
        w.sync()
        assert (info.fetch() == POISON).all() and (defer.fetch() == POISON).all()
        assert np.array_equal(gpu_resolve(w, keys), old), "a refused call changed the snapshot"
        # count == 0: the info alone
        defer, info = Out(w, 256), Out(w, 64)
        assert L.upe_gpu_neigh_learn(ctx, None, 0, defer.ptr, info.ptr, None) == 0
        x = info.fetch().view(LEARN_INFO_DTYPE)[0]
        assert _info(x) == (0, 0, 0, 0, 0, lc.NONE64, 0, 0)
        assert (defer.fetch() == POISON).all()
        assert w.launch_info() == before
        assert np.array_equal(gpu_resolve(w, keys), old)
        w.free(buf)
    image.free()

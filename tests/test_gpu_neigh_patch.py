"""upe_gpu_neigh_patch on the device against its host twin (upe_neigh_patch_host, pinned to the
reference's update by tests/test_neigh_patch.py), bit for bit: the tables of tests/neigh_cases.py
small and embedded with the records of tests/patch_cases.py, record counts around a wave and a
workgroup, many records racing for three slots, what a classify launch queued before and after a
patch reads, the L1 entries a patch must leave alone, and the state it must not touch.  The miss
list is poisoned before the call; what lies behind the missed ranks must keep the poison."""
from __future__ import annotations

import numpy as np
import pytest

import neigh_cases as nc
import oracle
import patch_cases as pc
import resolve_cases as rc
from test_gpu_keys import POISON, Out, dev_in
from test_gpu_parity import _force_dst
from test_gpu_resolve import gpu_resolve
from test_neigh_cases import check_against_reference, workload
from upe_amd import gpu, neigh
from upe_amd.layout import CTRL_WRITE_DTYPE, CW_ARP, CW_NDP, PATCH_INFO_DTYPE

pytestmark = pytest.mark.gpu

ROOM = 16   # entries behind the miss list that must keep the poison
NONE64 = (1 << 64) - 1
A = "embed:combo"
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513, 1025)


def _info(x):
    return tuple(int(x[f]) for f in ("records", "patched", "missed", "first_miss"))


def gpu_patch(w, recs, want_miss=True, stream=None):
    """(the missed ranks, info) of one upe_gpu_neigh_patch; the records must come back as they
    went in, and nothing past the missed ranks may be written."""
    n = len(recs)
    raw = np.ascontiguousarray(recs).view(np.uint8).ravel()
    dw = dev_in(w, raw)
    miss, info = Out(w, 4 * (n + ROOM)), Out(w, 32)
    w.neigh_patch(dw, n, miss.ptr if want_miss else None, info.ptr, stream)
    x = info.fetch().view(PATCH_INFO_DTYPE)[0]
    m = miss.fetch()
    missed = int(x["missed"]) if want_miss else 0
    assert (m[4 * missed:] == POISON).all(), "written past the missed ranks"
    after = np.empty(max(raw.size, 1), np.uint8)
    if raw.size:
        w.d2h(after[:raw.size], dw)
        w.sync()
        assert np.array_equal(after[:raw.size], raw), "d_writes was written"
    w.free(dw)
    return m[:4 * missed].view(np.uint32).copy(), x


def check(w, name, arp, ndp, recs, what):
    """Patch the loaded snapshot (of arp / ndp) and the twin's image with recs; answers, misses
    and info must agree."""
    keys = pc.address_keys(name, recs)
    image = gpu.NeighImage(arp, ndp)
    miss_h, info_h = gpu.neigh_patch_host(image, recs)
    want = gpu.neigh_image_lookup_host(image, rc.as_keys(keys))
    image.free()
    miss, info = gpu_patch(w, recs)
    assert _info(info) == _info(info_h), what
    assert np.array_equal(miss, miss_h), what
    got = gpu_resolve(w, keys)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} answers differ, first "
                           f"{int(bad[0])}: {int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}")
    return want, info_h


@pytest.mark.parametrize("name", pc.CASES + nc.BOUNDARY_CASES)
def test_tables(gpu_worker_factory, name):
    cs = nc.case(name)
    recs = pc.records(name if not name.startswith("boundary:") else "dup")
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        before = gpu_resolve(w, pc.address_keys(name, recs))
        want, info = check(w, name, cs.arp, cs.ndp, recs, name)
        # a second patch of the same records finds the owner words as the first left them
        check(w, name, *neigh.patch(cs.arp, cs.ndp, recs)[:2], recs, name + " again")
    assert _info(info)[2] > 0
    if _info(info)[1]:
        assert not np.array_equal(before, want), "the patch changed no answer"


def _sized(n):
    """n records cycling through case A's, each with its rank's MAC."""
    base = pc.records(A)
    w = base[np.arange(n) % len(base)].copy()
    for r in range(n):
        w["mac"][r] = np.frombuffer(pc.rank_mac(r, 0x51), np.uint8)
    return w


@pytest.mark.parametrize("n", COUNTS)
def test_sizes(gpu_worker_factory, n):
    cs = nc.case(A)
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        check(w, A, cs.arp, cs.ndp, _sized(n), f"count {n}")


def test_without_a_miss_list(gpu_worker_factory):
    cs, recs = nc.case(A), pc.records(A)
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        miss, info = gpu_patch(w, recs, want_miss=False)
        image = gpu.NeighImage(cs.arp, cs.ndp)
        _, info_h = gpu.neigh_patch_host(image, recs)
        keys = pc.address_keys(A, recs)
        assert _info(info) == _info(info_h) and len(miss) == 0
        assert np.array_equal(gpu_resolve(w, keys),
                              gpu.neigh_image_lookup_host(image, rc.as_keys(keys)))
        image.free()


def test_many_records_race_for_three_slots(gpu_worker_factory):
    """1025 records at 3 addresses, the MAC a function of the rank; a miss at every 64th rank.
    Each address's first record lies in the first wave of the first workgroup, its last in the
    last wave of the fourth; the record of highest rank must be the one that stays."""
    cs = nc.case(A)
    a4 = [k for k in cs.own("arp") if nc.Probe(cs.arp).slot(k) >= 0][:2]
    a6 = [k for k in cs.own("ndp") if nc.Probe(cs.ndp).slot(k) >= 0][:1]
    targets = [(CW_ARP, a4[0]), (CW_NDP, a6[0]), (CW_ARP, a4[1])]
    absent = (CW_ARP, 0xDEAD0001)
    n = 1025
    items = [absent if r % 64 == 0 else targets[r % 3] for r in range(n)]
    recs = pc.make(items, salt=0x77)
    last = {t: max(r for r in range(n) if items[r] == t) for t in targets}
    first = {t: min(r for r in range(n) if items[r] == t) for t in targets}
    for t in targets:
        assert first[t] // 64 != last[t] // 64 and first[t] // gpu.PATCH_BLOCK != last[t] // gpu.PATCH_BLOCK
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        _, info = check(w, A, cs.arp, cs.ndp, recs, "race")
        keys = rc.key_bytes([k for k, _ in targets], [a for _, a in targets],
                            np.random.default_rng(3))
        got = gpu_resolve(w, keys)
    assert _info(info) == (n, n - 17, 17, 0)
    for j, t in enumerate(targets):
        assert int(got[j]) == rc.mac_word(pc.rank_mac(last[t], 0x77)), (t, hex(int(got[j])))


# ---------------------------------------------------------------------------------------------
# what classify sees
# ---------------------------------------------------------------------------------------------

def _refresh_records(cs):
    """A new MAC for every address of the case's own that a probe reaches, and the case's other
    records (misses among them) in front."""
    items = [(int(k), bytes(ip) if k == CW_NDP else int.from_bytes(bytes(ip[:4]), "little"))
             for k, ip in zip(pc.records(cs.name)["kind"], pc.records(cs.name)["ip"])]
    for fam, kind in (("arp", CW_ARP), ("ndp", CW_NDP)):
        p = nc.Probe(cs.table(fam))
        items += [(kind, k) for k in cs.own(fam) if p.slot(k) >= 0]
    return pc.make(items, salt=0xC1)


def _run(b, emit):
    b.run_emit() if emit else b.run()


def _fetch(b, wl, emit):
    frames, verdict = b.fetch()
    if emit:
        frames = gpu.hdr_apply(frames, wl.desc, b.fetch_hdr())
    return frames, verdict


@pytest.mark.parametrize("emit", [False, True], ids=["in_place", "emit"])
@pytest.mark.parametrize("name", ["combo", "embed:combo"], ids=["staged", "memory"])
def test_classify_before_and_after(gpu_worker_factory, name, emit):
    """process, patch, process on one stream with no synchronisation between: the first batch is
    the reference worker's under the old tables, the second under the new ones."""
    cs, wl = nc.case(name), workload(name)
    recs = _refresh_records(cs)
    arp2, ndp2, _, info = neigh.patch(wl.arp, wl.ndp, recs)
    assert info[1] > 0 and info[2] > 0
    r1 = oracle.run_restated(wl)
    wl2 = wl.copy()
    wl2.arp, wl2.ndp, wl2.l1 = arp2, ndp2, r1.l1.copy()
    r2 = oracle.run_restated(wl2)
    check_against_reference(wl2, r2, name + " after the patch")
    old = wl.copy()
    old.l1 = r1.l1.copy()
    assert not np.array_equal(oracle.run_restated(old).frames, r2.frames), "the patch is not seen"
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        b1, b2 = gpu.DeviceBatch(w, wl.frames, wl.desc), gpu.DeviceBatch(w, wl.frames, wl.desc)
        raw = np.ascontiguousarray(recs).view(np.uint8).ravel()
        dw, di = dev_in(w, raw), w.malloc(32)
        _run(b1, emit)
        w.neigh_patch(dw, len(recs), None, di)
        _run(b2, emit)
        f1, v1 = _fetch(b1, wl, emit)
        f2, v2 = _fetch(b2, wl, emit)
        l1 = w.get_l1()
        for p in (dw, di):
            w.free(p)
        b1.free(), b2.free()
    assert np.array_equal(v1, r1.verdict) and np.array_equal(f1, r1.frames), "before the patch"
    assert np.array_equal(v2, r2.verdict), "after the patch"
    assert np.array_equal(f2, r2.frames), "after the patch"
    assert l1.tobytes() == r2.l1.tobytes()


@pytest.mark.parametrize("emit", [False, True], ids=["in_place", "emit"])
@pytest.mark.parametrize("name", ["combo", "embed:combo"], ids=["staged", "memory"])
def test_l1_entries_keep_the_old_mac(gpu_worker_factory, name, emit):
    """The L1 entries hold the addresses being refreshed: the reference never invalidates them,
    so packets aimed at an entry go on with the old MAC until another address replaces it."""
    cs = nc.case(name)
    wl = workload(name).copy()
    a4 = next(k for k in cs.own("arp") if k and nc.Probe(cs.arp).slot(k) >= 0)
    a6 = next(k for k in cs.own("ndp") if any(k) and nc.Probe(cs.ndp).slot(k) >= 0)
    l1 = wl.l1.copy()
    l1["last_arp_ip"] = a4
    l1["last_arp_mac"] = np.frombuffer(nc.Probe(cs.arp).mac(a4), np.uint8)
    l1["last_ndp_ip"] = np.frombuffer(a6, np.uint8)
    l1["last_ndp_mac"] = np.frombuffer(nc.Probe(cs.ndp).mac(a6), np.uint8)
    recs = pc.make([(CW_ARP, a4), (CW_NDP, a6)], salt=0xE1)
    wl.l1 = l1
    _force_dst(wl, 200, a4, np.frombuffer(a6, np.uint8))
    wl2 = wl.copy()
    wl2.arp, wl2.ndp, _, info = neigh.patch(wl.arp, wl.ndp, recs)
    assert info == (2, 2, 0, NONE64)
    r = oracle.run_restated(wl2)
    check_against_reference(wl2, r, name + " L1")
    assert not np.array_equal(r.frames, oracle.run_restated(wl).frames)
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)   # the old tables, the entries agreeing with them
        miss, _ = gpu_patch(w, recs)
        assert len(miss) == 0
        assert w.get_l1().tobytes() == l1.tobytes(), "the patch touched the L1 entries"
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        _run(b, emit)
        frames, verdict = _fetch(b, wl, emit)
        b.free()
        assert not w.launch_info()["variant"] & gpu.VAR_NOLB
        assert np.array_equal(verdict, r.verdict)
        assert np.array_equal(frames, r.frames)
        assert w.get_l1().tobytes() == r.l1.tobytes()


# ---------------------------------------------------------------------------------------------
# what a patch leaves alone
# ---------------------------------------------------------------------------------------------

def test_untouched_state(gpu_worker_factory):
    cs, wl = nc.case(A), workload(A)
    recs = pc.records(A)
    keys = pc.address_keys(A, recs)
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        gpu.run_workload(wl, worker=w)
        image = gpu.NeighImage(cs.arp, cs.ndp)
        w.load_neigh_image(image)
        old = gpu_resolve(w, keys)

        def state():
            c, s = w.get_stats()
            return c.tobytes(), s.tobytes(), w.get_latency().tobytes(), w.launch_info()

        before = state()
        _, info = gpu_patch(w, recs)
        assert int(info["patched"]) > 0
        assert state() == before
        assert not np.array_equal(gpu_resolve(w, keys), old)
        # the image is a value: the dry run still answers with the old MACs
        assert np.array_equal(gpu_resolve(w, keys, image=image), old)
        image.free()


def test_argument_errors_and_empty(gpu_worker_factory):
    L = gpu.LIB
    cs = nc.case(A)
    with gpu_worker_factory(16) as w:
        c = w._ctx
        w.load_neigh(cs.arp, cs.ndp)
        keys = pc.address_keys(A, pc.records(A))
        old = gpu_resolve(w, keys)
        buf = dev_in(w, np.ascontiguousarray(pc.records(A)).view(np.uint8).ravel())
        miss, info = Out(w, 256), Out(w, 32)
        before = w.launch_info()
        assert L.upe_gpu_neigh_patch(None, buf, 1, miss.ptr, info.ptr, None) == -1
        assert b"null context" in L.upe_gpu_last_error()
        for args in ((c, buf, 1, miss.ptr, None, None), (c, None, 1, miss.ptr, info.ptr, None)):
            assert L.upe_gpu_neigh_patch(*args) == -1
            assert b"null buffer" in L.upe_gpu_last_error()
        assert L.upe_gpu_neigh_patch(c, buf + 8, 1, miss.ptr, info.ptr, None) == -1
        assert b"aligned" in L.upe_gpu_last_error()
        assert L.upe_gpu_neigh_patch(c, buf, (1 << 32) - gpu.PATCH_BLOCK, miss.ptr, info.ptr,
                                     None) == -1
        assert b"32 bits" in L.upe_gpu_last_error()
        w.sync()
        assert (info.fetch() == POISON).all() and (miss.fetch() == POISON).all()
        assert np.array_equal(gpu_resolve(w, keys), old), "a refused call changed the snapshot"
        # count == 0: the info alone
        miss, info = Out(w, 256), Out(w, 32)
        assert L.upe_gpu_neigh_patch(c, None, 0, miss.ptr, info.ptr, None) == 0
        x = info.fetch().view(PATCH_INFO_DTYPE)[0]
        assert _info(x) == (0, 0, 0, NONE64)
        assert (miss.fetch() == POISON).all()
        assert w.launch_info() == before
        assert np.array_equal(gpu_resolve(w, keys), old)
        w.free(buf)

"""upe_gpu_resolve_keys on the device against its numpy mirror (upe_amd/neigh.py, pinned to the
probe model and to the reference by tests/test_resolve.py), bit for bit: every size around a wave,
a workgroup and a ragged last tile, with the families alternating per lane and in runs of a wave;
the adversarial tables of tests/neigh_cases.py small and embedded; the dry run of a compiled image
beside a loaded snapshot; the snapshot loaded in two halves.  Every output buffer is poisoned
before the call and followed by a canary that must survive it (tests/test_gpu_keys.py's Out)."""
from __future__ import annotations

import numpy as np
import pytest

import neigh_cases as nc
import oracle
import resolve_cases as rc
from test_gpu_keys import POISON, Out, dev_in
from test_gpu_parity import _assert_same, _force_dst
from test_neigh_cases import as_ref, oracle_of, workload
from upe_amd import gpu, neigh, synth

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 256, 257, 4096 + 37)
A, B = "embed:combo", "dup"   # a loaded snapshot and another one


def gpu_resolve(w, kb, image=None):
    """d_mac of the key records kb (n, 44); the keys buffer must come back as it went in."""
    n = len(kb)
    dk = dev_in(w, kb)
    out = Out(w, 8 * n)
    w.resolve_keys(dk, n, out.ptr, image=image)
    got = out.fetch().view(np.uint64).copy()
    after = np.empty(max(kb.size, 1), np.uint8)
    if kb.size:
        w.d2h(after[:kb.size], dk)
        w.sync()
        assert np.array_equal(after[:kb.size], np.ascontiguousarray(kb).ravel()), "d_keys was written"
    w.free(dk)
    return got


def check(w, cs, kb, what, image=None):
    want = neigh.resolve_keys(cs.arp, cs.ndp, rc.as_keys(kb))
    got = gpu_resolve(w, kb, image)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} differ, first {int(bad[0])} "
                           f"(ip_ver {int(kb[bad[0], 0])}): {int(got[bad[0]]):#x} vs "
                           f"{int(want[bad[0]]):#x}")
    return want


def _sized(n, runs):
    """n keys of case A's queries: IPv4 and IPv6 alternate per lane, or in runs of 64."""
    kb, fams, _, _ = rc.queries(A)
    f = np.array(fams)
    k4, k6 = kb[f == "arp"], kb[f == "ndp"]
    i = np.arange(n)
    is6 = (i // 64 if runs else i) % 2 == 1
    out = np.empty((n, 44), np.uint8)
    out[~is6] = k4[np.arange(int((~is6).sum())) % len(k4)]
    out[is6] = k6[np.arange(int(is6.sum())) % len(k6)]
    return out


@pytest.mark.parametrize("runs", [False, True], ids=["alternating", "runs64"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu_worker_factory, n, runs):
    cs = nc.case(A)
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        want = check(w, cs, _sized(n, runs), f"n={n} runs={runs}")
    assert n < 64 or ((want != 0).any() and (want == 0).any())


def test_one_workgroup_walks_every_tile(gpu_worker_factory, monkeypatch):
    monkeypatch.setenv("UPE_GPU_GRID_CAP", "1")
    cs = nc.case(A)
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        for runs in (False, True):
            check(w, cs, _sized(4096 + 37, runs), f"grid cap 1, runs={runs}")


@pytest.mark.parametrize("name", rc.CASES)
def test_tables(gpu_worker_factory, name):
    cs = nc.case(name)
    kb, fams, _, groups = rc.queries(name)
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        want = check(w, cs, kb, name)
    if name.startswith("boundary:"):   # 1638 entries start at 2048 index slots, 1639 at 4096
        _, fam, which = name.split(":")
        assert len(nc.anatomy(cs.table(fam))["reachable"]) == nc.BOUNDARY_N + (which == "n1")
    g, f = np.array(groups), np.array(fams)
    assert not want[g == "flip"].any()
    for fam in ("arp", "ndp"):
        if nc.anatomy(cs.table(fam))["reachable"]:
            assert want[(f == fam) & (g == "stored")].any(), (name, fam)


def test_empty_tables_answer_zero(gpu_worker_factory):
    kb = _sized(600, False)
    invalid = nc.case(A)
    arp, ndp = invalid.arp.copy(), invalid.ndp.copy()
    arp["valid"], ndp["valid"] = 0, 0   # the addresses are still there: nothing valid
    with gpu_worker_factory(16) as w:
        assert not gpu_resolve(w, kb).any(), "a fresh context"
        w.load_neigh(None, None)
        assert not gpu_resolve(w, kb).any(), "capacity 0"
        w.load_neigh(arp, ndp)
        assert not gpu_resolve(w, kb).any(), "nothing valid"
        assert not neigh.resolve_keys(arp, ndp, rc.as_keys(kb)).any()


def test_other_ip_versions_and_union_bytes(gpu_worker_factory):
    cs = nc.case(A)
    _, fams, addrs, _ = rc.queries(A)
    fams, addrs = list(fams[:300]), list(addrs[:300])
    vers = [4 if f == "arp" else 6 for f in fams]
    rng = np.random.default_rng(8)
    dirty = rc.key_bytes(fams, addrs, rng)
    clean = rc.key_bytes(fams, addrs, rng, clean4=True)
    other = rc.key_bytes([(0, 5, 255)[i % 3] for i in range(300)], addrs, rng)
    assert vers.count(4) and dirty[np.array(vers) == 4, 24:36].any()
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        want = check(w, cs, dirty, "noise behind IPv4 addresses")
        assert np.array_equal(check(w, cs, clean, "zeros behind IPv4 addresses"), want)
        assert want.any() and not gpu_resolve(w, other).any()


# ---------------------------------------------------------------------------------------------
# the dry run
# ---------------------------------------------------------------------------------------------

def _state(w):
    c, s = w.get_stats()
    return c.tobytes(), s.tobytes(), w.get_l1().tobytes(), w.launch_info()


def _classify(w, wl):
    got = gpu.run_workload(wl, worker=w)
    return got


def test_dry_run_leaves_the_context_alone(gpu_worker_factory):
    wl, ref = workload(A), as_ref(oracle_of(A))
    ca, cb = nc.case(A), nc.case(B)
    # both cases' queries against both tables: each table's own addresses hit only there
    kb = np.concatenate([rc.queries(A)[0], rc.queries(B)[0]])
    want_a = neigh.resolve_keys(ca.arp, ca.ndp, rc.as_keys(kb))
    want_b = neigh.resolve_keys(cb.arp, cb.ndp, rc.as_keys(kb))
    assert not np.array_equal(want_a, want_b) and want_a.any() and want_b.any()
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        before = _state(w)
        image = gpu.NeighImage(cb.arp, cb.ndp)
        for _ in range(2):   # the image is not consumed
            assert np.array_equal(gpu_resolve(w, kb, image=image), want_b), "the dry run"
        assert np.array_equal(gpu_resolve(w, kb), want_a), "the loaded snapshot is still A"
        assert _state(w) == before
        _assert_same(_classify(w, wl), ref, "a batch under A after the dry run")
        assert w.launch_info()["launches"] == before[3]["launches"] + 1
        # and the image still loads
        w.load_neigh_image(image)
        assert np.array_equal(gpu_resolve(w, kb), want_b)
        image.free()


# ---------------------------------------------------------------------------------------------
# the two halves
# ---------------------------------------------------------------------------------------------

def test_load_image_equals_load_neigh(gpu_worker_factory):
    wl, ref = workload(A), as_ref(oracle_of(A))
    got = []
    for halves in (False, True):
        with gpu_worker_factory(wl.capacity) as w:
            w.load_rules(wl.rules_sorted)
            if halves:
                image = gpu.NeighImage(wl.arp, wl.ndp)
                w.load_neigh_image(image)
                image.free()
            else:
                w.load_neigh(wl.arp, wl.ndp)
            w.set_port(wl.eth_addr, wl.ip4_addr)
            w.set_l1(wl.l1)
            got.append(_classify(w, wl))
    _assert_same(got[1], ref, "load_neigh_image(compile(A))")
    _assert_same(got[0], ref, "load_neigh(A)")
    for x, y in zip(got[0], got[1]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_failing_load_keeps_the_snapshot(gpu_worker_factory):
    cs = nc.case(A)
    kb = rc.queries(A)[0]
    L = gpu.LIB
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        want = check(w, cs, kb, "before")
        before = w.launch_info()
        assert L.upe_gpu_load_neigh_image(w._ctx, None) == -1
        assert b"null neighbour image" in L.upe_gpu_last_error()
        image = gpu.NeighImage(None, None)
        assert L.upe_gpu_load_neigh_image(None, image.ptr) == -1
        assert b"null context" in L.upe_gpu_last_error()
        image.free()
        assert w.launch_info() == before
        assert np.array_equal(gpu_resolve(w, kb), want) and want.any(), "A still answers"


def test_lookback_returns_after_load_image(gpu_worker_factory, monkeypatch):
    """Agreement reached (the kernel without look-back), then a snapshot loaded through
    load_neigh_image: the next launch runs the look-back again.  Then the same with a snapshot
    that gives the L1 entry's address another MAC and a set_l1 that keeps the old one: the
    look-back variant, and the oracle's answers under the new tables."""
    monkeypatch.setenv("UPE_GPU_LB_SYNC", "1")
    wl = synth.config_b(n=20_000, seed=32)

    def one(w, x):
        b = gpu.DeviceBatch(w, x.frames, x.desc)
        b.run()
        out = b.fetch()
        b.free()
        return out

    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        for _ in range(3):
            one(w, wl)
        assert w.launch_info()["variant"] & gpu.VAR_NOLB
        image = gpu.NeighImage(wl.arp, wl.ndp)
        w.load_neigh_image(image)
        image.free()
        one(w, wl)
        assert not w.launch_info()["variant"] & gpu.VAR_NOLB
        for _ in range(2):
            one(w, wl)
        assert w.launch_info()["variant"] & gpu.VAR_NOLB
        # the entry's address under another MAC in the new snapshot; the entry keeps the old one
        l1 = w.get_l1()
        ip = int(l1["last_arp_ip"][0])
        wl2 = wl.copy()
        slot = int(np.nonzero((wl2.arp["valid"] == 1) & (wl2.arp["ip"] == ip))[0][0])
        wl2.arp["mac"][slot] = np.frombuffer(bytes.fromhex("0e0e0e0e0e0e"), np.uint8)
        assert wl2.arp["mac"][slot].tobytes() != l1["last_arp_mac"][0].tobytes()
        wl2.l1 = l1.copy()
        _force_dst(wl2, 3_000, ip)
        image = gpu.NeighImage(wl2.arp, wl2.ndp)
        w.load_neigh_image(image)
        image.free()
        w.set_l1(l1)
        frames, verdict = one(w, wl2)
        assert not w.launch_info()["variant"] & gpu.VAR_NOLB
        r2 = oracle.run_restated(wl2)
        assert np.array_equal(verdict, r2.verdict)
        assert np.array_equal(frames, r2.frames)
        assert w.get_l1().tobytes() == r2.l1.tobytes()


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing(gpu_worker_factory):
    L = gpu.LIB
    with gpu_worker_factory(16) as w:
        c = w._ctx
        buf = w.malloc(4096)
        guard = Out(w, 64)
        before = w.launch_info()
        assert L.upe_gpu_resolve_keys(None, None, buf, 1, guard.ptr, None) == -1
        assert b"null context" in L.upe_gpu_last_error()
        for args in ((c, None, None, 1, guard.ptr, None), (c, None, buf, 1, None, None)):
            assert L.upe_gpu_resolve_keys(*args) == -1
            assert b"null buffer" in L.upe_gpu_last_error()
        assert L.upe_gpu_resolve_keys(c, None, buf, 1 << 32, guard.ptr, None) == -1
        assert b"32 bits" in L.upe_gpu_last_error()
        assert L.upe_gpu_resolve_keys(c, None, buf, 1, guard.ptr + 4, None) == -1
        assert b"aligned" in L.upe_gpu_last_error()
        # n == 0 is a no-op, whatever the buffers
        assert L.upe_gpu_resolve_keys(c, None, None, 0, None, None) == 0
        assert w.launch_info() == before
        assert (guard.fetch() == POISON).all(), "a refused call wrote its output"
        w.free(buf)

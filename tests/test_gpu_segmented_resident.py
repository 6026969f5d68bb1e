"""upe_gpu_process_segmented_resident against upe_gpu_process_segmented, output for output, and
against the reference worker: the control batches of tests/test_gpu_control.py, a batch whose
control packets only refresh known neighbours (no rebuild at all), a batch that teaches an address
and then refreshes it, and a batch without control packets."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from test_gpu_control import KEEP, _expected, _rows, _segmented, with_control
from test_gpu_parity import _assert_same
from upe_amd import gpu, neigh, synth
from upe_amd.layout import CW_ARP, V_FWD

pytestmark = pytest.mark.gpu
NOW = 1234


def _resident(worker_factory, wl):
    w = worker_factory(wl.capacity)
    try:
        w.configure(wl)
        arp, ndp = wl.arp.copy(), wl.ndp.copy()
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        info = w.process_segmented_resident(b.frames, b.desc, b.verdict, b.n, arp, ndp, now=NOW)
        frames, verdict = b.fetch()
        b.free()
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    return (frames, verdict, counters, stats, l1), arp, ndp, info


def _ref(r):
    return {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
            "rule_stats": r.rule_stats, "l1": r.l1}


def _both(gpu_worker_factory, wl, what):
    """Both calls on fresh contexts and copies of the host arrays: every output equal."""
    old, arp_o, ndp_o, writes = _segmented(gpu_worker_factory, wl)
    new, arp_n, ndp_n, info = _resident(gpu_worker_factory, wl)
    for x, y, field in zip(old, new, ("frames", "verdict", "counters", "rule_stats", "l1")):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"{what}: {field}"
    # the slot arrays field by field, update_at included (the padding between fields is nobody's)
    for f in KEEP + ["update_at"]:
        assert np.array_equal(arp_o[f], arp_n[f]) and np.array_equal(ndp_o[f], ndp_n[f]), (what, f)
    assert int(info["writes"]) == writes
    assert int(info["patched"]) + int(info["rebuilds"]) == writes
    return new, arp_n, ndp_n, info


def _derived(wl):
    """(patched, rebuilds) numpy derives: neigh.patch record by record over the tables as the
    writes leave them."""
    recs, _ = gpu.ctrl_writes_host(wl.frames, wl.desc)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    patched = rebuilds = 0
    for j in range(len(recs)):
        if not len(arp if recs["kind"][j] == CW_ARP else ndp):
            continue
        if neigh.patch(arp, ndp, recs[j:j + 1])[3][1]:
            patched += 1
        else:
            rebuilds += 1
        gpu.neigh_apply_writes(arp, ndp, recs[j:j + 1], NOW)
    return patched, rebuilds


@pytest.mark.parametrize("seed,n,k", [(31, 4000, 40), (32, 20000, 200), (33, 60000, 7)])
def test_parity_with_the_segmented_call(gpu_worker_factory, seed, n, k):
    wl = with_control(synth.config_c(n=n, seed=seed), k, seed)
    got, arp, ndp, info = _both(gpu_worker_factory, wl, f"seed {seed}")
    r = _expected(wl)
    _assert_same(got, _ref(r), f"seed {seed}", batch_relative=True)
    assert np.array_equal(arp[KEEP], r.arp[KEEP]) and np.array_equal(ndp[KEEP], r.ndp[KEEP])
    assert (int(info["patched"]), int(info["rebuilds"])) == _derived(wl)
    assert int(info["ctrl"]) >= int(info["writes"]) > 0


def _with_arp(wl, teach, every):
    """wl with one ARP packet per (address, mac) of `teach` put in front of every `every`-th
    packet, so that forwarded traffic follows each."""
    h, lens = _rows(wl)
    rows, lns, src = [], [], 0
    for j, (ip, mac) in enumerate(teach):
        p = min(j * every, wl.n)
        rows.append(h[src:p])
        lns.append(lens[src:p])
        f = synth._frame(synth._eth(0x0806, dst=b"\xff" * 6),
                         synth._arp(1, mac, ip, bytes(6), 0x0A800001))
        r = np.zeros((1, 128), np.uint8)
        r[0, :len(f)] = np.frombuffer(f, np.uint8)
        rows.append(r)
        lns.append(np.array([len(f)], np.int64))
        src = p
    rows.append(h[src:])
    lns.append(lens[src:])
    frames, desc = synth.pack_frames(np.concatenate(rows), np.concatenate(lns))
    return synth.Workload(wl.name + "+arp", frames, desc, wl.rules, wl.capacity, wl.arp.copy(),
                          wl.ndp.copy(), wl.eth_addr, wl.ip4_addr, wl.l1.copy())


def _v4_destinations(wl):
    h, _ = _rows(wl)
    v4 = ((h[:, 12].astype(np.int64) << 8) | h[:, 13]) == 0x0800
    return (h[v4, 30:34].astype(np.int64) * np.array([1 << 24, 1 << 16, 1 << 8, 1])).sum(axis=1)


def test_refresh_only_batch(gpu_worker_factory):
    """4096 packets, 64 of them ARP packets from addresses the table holds, with new MACs, each
    followed by traffic to those addresses: 64 patches and no rebuild."""
    base = synth.config_c(n=4096 - 64, seed=41)
    known = set(int(x) for x in base.arp["ip"][base.arp["valid"] != 0])
    h, _ = _rows(base)
    v4 = ((h[:, 12].astype(np.int64) << 8) | h[:, 13]) == 0x0800
    dst = (h[:, 30:34].astype(np.int64) * np.array([1 << 24, 1 << 16, 1 << 8, 1])).sum(axis=1)
    fwd = (oracle.run_restated(base).verdict & 0xF) == V_FWD
    # packets that are forwarded to an address the table holds: ARP packet j, put in front of
    # packet 63 j, refreshes the destination of the first of them at or behind that place
    cand = np.nonzero(v4 & fwd & np.isin(dst, list(known)))[0]
    assert len(cand) >= 8
    pick = [int(dst[cand[min(np.searchsorted(cand, 63 * j), len(cand) - 1)]]) for j in range(64)]
    teach = [(ip, bytes([0x0C, j, 1, 2, 3, 4])) for j, ip in enumerate(pick)]
    wl = _with_arp(base, teach, 63)
    assert wl.n == 4096
    got, arp, ndp, info = _both(gpu_worker_factory, wl, "refresh only")
    assert (int(info["writes"]), int(info["patched"]), int(info["rebuilds"])) == (64, 64, 0)
    assert _derived(wl) == (64, 0)
    r = _expected(wl)
    _assert_same(got, _ref(r), "refresh only", batch_relative=True)
    assert np.array_equal(arp[KEEP], r.arp[KEEP])
    assert not np.array_equal(oracle.run_restated(wl, apply_control=False).frames, r.frames)


def test_new_then_refreshed(gpu_worker_factory):
    """New and known addresses mixed; a new address is taught (a rebuild) and later refreshed (a
    patch)."""
    base = synth.config_c(n=6000, seed=43)
    known = set(int(x) for x in base.arp["ip"][base.arp["valid"] != 0])
    dst = _v4_destinations(base)
    old = [int(d) for d in dst if int(d) in known][:6]
    new = sorted(set(int(d) for d in dst if int(d) not in known))[:3]
    if not new:   # every destination is known: addresses nobody is sent to do as well
        new = [0x0AFE0001, 0x0AFE0002, 0x0AFE0003]
    order = [new[0], old[0], new[0], old[1], new[1], old[0], new[1], new[2 % len(new)], old[2]]
    teach = [(ip, bytes([0x0D, j, 9, 9, 9, j])) for j, ip in enumerate(order)]
    wl = _with_arp(base, teach, 500)
    got, arp, ndp, info = _both(gpu_worker_factory, wl, "mixed")
    want = _derived(wl)
    assert (int(info["patched"]), int(info["rebuilds"])) == want
    assert want[0] >= 5 and want[1] >= 2
    r = _expected(wl)
    _assert_same(got, _ref(r), "mixed", batch_relative=True)
    assert np.array_equal(arp[KEEP], r.arp[KEEP])


def test_no_control_packets(gpu_worker_factory):
    wl = synth.config_b(n=50000, seed=8)
    got, arp, ndp, info = _resident(gpu_worker_factory, wl)
    plain = gpu.run_workload(wl)
    for x, y in zip(got, plain):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert info.tobytes() == bytes(32)
    assert np.array_equal(arp, wl.arp) and np.array_equal(ndp, wl.ndp)


def test_empty_batch(gpu_worker_factory):
    wl = synth.config_b(n=16, seed=8)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        dev = w.malloc(256)
        info = w.process_segmented_resident(dev, dev, dev, 0, wl.arp.copy(), wl.ndp.copy())
        assert info.tobytes() == bytes(32)
        w.free(dev)
    finally:
        w.close()

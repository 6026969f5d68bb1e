"""Every device buffer a context grows on demand, grown on one context: each entry point runs at
a small size, then at one past the room the small run left, and the larger run is checked
bit-exactly against the oracle (a regrown buffer that is too small, stale, or not republished to
the device state shows as a wrong answer or a fault).  Then the context is closed, and a second
one opened and closed without a batch."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
from test_gpu_control import KEEP, with_control
from test_gpu_control import _expected as control_expected
from test_gpu_egress_pack import Out as PackOut
from test_gpu_egress_pack import _check as pack_check
from test_gpu_host import _check as check_host
from test_gpu_parity import _assert_same
from test_gpu_rx_dispatch import _check as rx_check
from test_gpu_rx_dispatch import _dispatch as rx_run
from upe_amd import egress, gpu, synth
from upe_amd.layout import V_FWD, desc_lens, desc_offsets

pytestmark = pytest.mark.gpu

SMALL, LARGE = 64, 18_000   # one tile (room for 17 is allocated), then 18 tiles


def _ref(r):
    return {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
            "rule_stats": r.rule_stats, "l1": r.l1}


def _setup(w, wl):
    """wl's tables, identity and starting state on a context that has run other work."""
    w.reload_rules(wl.rules_sorted, capacity=wl.capacity, want_old=False)
    w.load_neigh(wl.arp, wl.ndp)
    w.set_port(wl.eth_addr, wl.ip4_addr)
    w.set_l1(wl.l1)
    w.reset_stats()


def _classify(w, wl, n):
    """The first n packets in place; the batch stays on the device."""
    b = gpu.DeviceBatch(w, wl.frames, wl.desc[:n])
    b.run()
    frames, verdict = b.fetch()
    counters, stats = w.get_stats()
    return b, (frames, verdict, counters, stats, w.get_l1())


def _hashes(wl):
    """The reference's parse result and flow hash per packet."""
    lib = oracle.oracle_lib()
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    hashes, ok = np.zeros(wl.n, np.uint32), np.zeros(wl.n, bool)
    for i in range(wl.n):
        rc, key = oracle.parse(bytes(wl.frames[offs[i]:offs[i] + min(int(lens[i]), 2048)]),
                               int(lens[i]))
        if rc == 0:
            ok[i] = True
            hashes[i] = lib.upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p))
    return hashes, ok


def _compact(w, b, n, want_verdict):
    index, count = w.malloc(4 * n), w.malloc(8)
    w.compact(b.verdict, n, V_FWD, index, count)
    h_index, h_count = np.zeros(n, np.uint32), np.zeros(1, np.uint64)
    w.sync()
    w.d2h(h_index, index)
    w.d2h(h_count, count)
    w.sync()
    for p in (index, count):
        w.free(p)
    want = np.nonzero((want_verdict[:n] & 0xF) == V_FWD)[0]
    assert int(h_count[0]) == want.size and want.size > 0
    assert np.array_equal(h_index[:want.size], want), f"compact of {n}"


def _rx_dispatch(w, b, n, wl, hashes, ok):
    got = rx_run(w, b, n, 4, 3)
    rx_check(got, hashes[:n], ok[:n], wl.desc[:n], 4, 3, f"rx_dispatch of {n}")


def _egress_pack(w, b, n, wl, r):
    """b was classified in place: its frames are the oracle's rewritten ones."""
    want = egress.pack_host(r.frames, wl.desc[:n], r.verdict[:n])
    room = int(want[3]["need"])
    assert int(want[3]["packed"]) > 0
    o = PackOut(w, n, room)
    try:
        w.egress_pack(b.frames, b.desc, b.verdict, n, o.out, room, o.desc, o.info,
                      out_index=o.index)
        pack_check(o.fetch(), want, room, f"egress_pack of {n}")
    finally:
        o.free()


def _marked(wl):
    """Packets upe_gpu_process_segmented gathers: ARP over Ethernet / IPv4, and NS / NA."""
    m = 0
    for o, ln in zip(desc_offsets(wl.desc), desc_lens(wl.desc)):
        p = wl.frames[o:o + 64]
        et = int(p[12]) << 8 | int(p[13])
        if et == 0x0806:
            m += p[14:20].tolist() == [0, 1, 8, 0, 6, 4]
        elif et == 0x86DD:
            m += ln >= 78 and p[20] == 58 and p[54] in (135, 136)
    return m


def _segmented(w, wl):
    _setup(w, wl)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    b = gpu.DeviceBatch(w, wl.frames, wl.desc)
    w.process_segmented(b.frames, b.desc, b.verdict, b.n, arp, ndp, now=1234)
    frames, verdict = b.fetch()
    b.free()
    counters, stats = w.get_stats()
    return (frames, verdict, counters, stats, w.get_l1()), arp, ndp


def _host_emit(w, wl, n):
    frames, verdict = wl.frames.copy(), np.zeros(n, np.uint32)
    rec = np.zeros((n, 16), np.uint8)
    w.process_host_emit(frames, wl.desc[:n].copy(), verdict, rec, 64, 0)
    return frames, verdict


def test_every_growing_buffer(gpu_worker_factory, monkeypatch):
    wl_b = synth.config_b(n=LARGE, seed=7)
    w = gpu_worker_factory(wl_b.capacity)
    try:
        # look-back flags and deferred candidates (17 tiles of room, then 18 tiles), in place
        r = oracle.run_restated(wl_b)
        hashes, ok = _hashes(wl_b)
        _setup(w, wl_b)
        b, _ = _classify(w, wl_b, SMALL)
        # the compaction's block counts and the dispatch's and the pack's tile tables
        _compact(w, b, SMALL, r.verdict)
        _rx_dispatch(w, b, SMALL, wl_b, hashes, ok)
        _egress_pack(w, b, SMALL, wl_b, r)
        b.free()
        _setup(w, wl_b)
        b, got = _classify(w, wl_b, LARGE)
        _assert_same(got, _ref(r), "config B, 18 tiles")
        _compact(w, b, LARGE, r.verdict)
        _rx_dispatch(w, b, LARGE, wl_b, hashes, ok)
        _egress_pack(w, b, LARGE, wl_b, r)
        b.free()

        # the group-by's keys and partials: a linear table past the LDS bins
        monkeypatch.setenv("UPE_GPU_TSS", "0")
        monkeypatch.setenv("UPE_GPU_TREE", "0")
        wl_d = synth.config_d(n=LARGE, seed=91, n_rules=4100)
        _setup(w, wl_d)
        assert w.rule_index_kind() == 0
        b, _ = _classify(w, wl_d, SMALL)
        b.free()
        _setup(w, wl_d)
        b, got = _classify(w, wl_d, LARGE)
        b.free()
        _assert_same(got, _ref(oracle.run_restated(wl_d)), "4100 linear rules")
        assert got[3]["packets"].sum() > 0

        # the control packets' marks (per packet) and gathered windows (per control packet)
        few = with_control(synth.config_c(n=500, seed=42), 1, 42)
        more = with_control(synth.config_c(n=2000, seed=42), 5, 42)
        assert (_marked(few), _marked(more)) == (1, 5)
        _segmented(w, few)
        got, arp, ndp = _segmented(w, more)
        want = control_expected(more)
        _assert_same(got, _ref(want), "5 control packets", batch_relative=True)
        assert np.array_equal(arp[KEEP], want.arp[KEEP]) and np.array_equal(ndp[KEEP], want.ndp[KEEP])

        # the host round trip's device slots
        wl_c = synth.config_c(n=4096, seed=23)
        _setup(w, wl_c)
        _host_emit(w, wl_c, 256)
        _setup(w, wl_c)
        frames, verdict = _host_emit(w, wl_c, wl_c.n)
        check_host(w, wl_c, frames, verdict, _ref(oracle.run_restated(wl_c)), "host emit, 4096")
    finally:
        w.close()
    gpu_worker_factory(16).close()

"""GPU: upe_gpu_rx_dispatch, the RX thread's dispatch of a batch to the worker rings (reference
src/rx_pcap.c:19-25,67-80) on the device: flow-hash ring for a packet that parses, the round-robin
cursor for every other packet, each ring's packets in arrival order.  Expected values come from
rx.dispatch_host over the reference's own parse results (tests/golden/flow_hash.npz, or
oracle.parse + upe_ref_flow_hash per packet), and, end to end, from one reference worker per ring
fed in RX order."""
from __future__ import annotations

import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import golden_io
import oracle
from upe_amd import gpu, rx, synth
from upe_amd.layout import desc_lens, desc_offsets

pytestmark = pytest.mark.gpu

B = gpu.RX_BLOCK   # packets per workgroup of the dispatch kernels
CASES = ["config_a", "config_b_small", "config_c_small", "config_cf_small", "config_d_small",
         "edge_zero", "ndp_walk"]


class Out:
    """Device outputs of one dispatch, poisoned before the call, fetched after it."""

    def __init__(self, w, n, rings, flow_hash=True, desc_out=True):
        self.w, self.n, self.rings = w, n, rings
        m = max(n, 1)
        self.ring, self.index = w.malloc(4 * m), w.malloc(4 * m)
        self.flow_hash = w.malloc(4 * m) if flow_hash else 0
        self.desc_out = w.malloc(8 * m) if desc_out else 0
        self.counts = w.malloc(8 * (rings + 1))
        for p, size in ((self.ring, 4 * m), (self.index, 4 * m), (self.flow_hash, 4 * m),
                        (self.desc_out, 8 * m), (self.counts, 8 * (rings + 1))):
            if p:
                w.h2d(p, np.full(size, 0xA5, np.uint8))
        w.sync()

    def fetch(self):
        w, n = self.w, self.n
        w.sync()
        got = {"ring": np.zeros(n, np.uint32), "index": np.zeros(n, np.uint32),
               "flow_hash": np.zeros(n, np.uint32), "desc_out": np.zeros(n, np.uint64),
               "counts": np.zeros(self.rings + 1, np.uint64)}
        for k, p in (("ring", self.ring), ("index", self.index), ("flow_hash", self.flow_hash),
                     ("desc_out", self.desc_out), ("counts", self.counts)):
            if p and got[k].size:
                w.d2h(got[k], p)
        w.sync()
        return got

    def free(self):
        for p in (self.ring, self.index, self.flow_hash, self.desc_out, self.counts):
            if p:
                self.w.free(p)


def _dispatch(w, b, n, rings, rr, **kw):
    o = Out(w, n, rings, **kw)
    try:
        w.rx_dispatch(b.frames, b.desc, n, rings, rr, o.ring, o.index, o.counts,
                      flow_hash=o.flow_hash, desc_out=o.desc_out)
        return o.fetch()
    finally:
        o.free()


def _check(got, hashes, ok, desc, rings, rr, what=""):
    ring, index, counts, _ = rx.dispatch_host(hashes, ok, rings, rr)
    assert np.array_equal(got["counts"], counts), f"{what}: counts {got['counts']} vs {counts}"
    bad = np.nonzero(got["ring"] != ring)[0]
    assert bad.size == 0, (f"{what}: {bad.size} ring ids differ, first {bad[:8].tolist()}: "
                           f"gpu {[hex(x) for x in got['ring'][bad[:8]]]} "
                           f"want {[hex(x) for x in ring[bad[:8]]]}")
    assert np.array_equal(got["index"], index), f"{what}: the per-ring lists differ"
    assert np.array_equal(got["flow_hash"], np.where(ok.astype(bool), hashes, 0)), what
    assert np.array_equal(got["desc_out"], desc[index]), f"{what}: desc_out != desc[index]"


@pytest.mark.parametrize("rings", [1, 2, 4, 64])
@pytest.mark.parametrize("case", CASES)
def test_golden_cases(gpu_worker_factory, case, rings):
    wl, _ = golden_io.load(case)
    hashes, ok = golden_io.flow_hash(case)
    w = gpu_worker_factory(wl.capacity)
    try:
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        for rr in (0, 3):
            got = _dispatch(w, b, wl.n, rings, rr)
            _check(got, hashes, ok, wl.desc, rings, rr, f"{case} rings {rings} rr {rr}")
        frames, _ = b.fetch()
        b.free()
    finally:
        w.close()
    assert np.array_equal(frames, wl.frames), "the dispatch wrote to the frames"


@functools.lru_cache(maxsize=None)
def _draw_d():
    """A config-D draw (about 10 % malformed; IPv4 options, truncations) and the reference's
    parse result and hash per packet, as tests/test_gpu_rss_egress.py::_expected_hashes."""
    wl = synth.config_d(n=3 * B + 17, seed=61, n_rules=256)
    lib = oracle.oracle_lib()
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    hashes, ok = np.zeros(wl.n, np.uint32), np.zeros(wl.n, bool)
    for i in range(wl.n):
        fr = bytes(wl.frames[offs[i]:offs[i] + min(int(lens[i]), 2048)])
        rc, key = oracle.parse(fr, int(lens[i]))
        if rc == 0:
            ok[i] = True
            hashes[i] = lib.upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p))
    return wl, hashes, ok


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17])
def test_boundaries(gpu_worker_factory, n):
    wl, hashes, ok = _draw_d()
    assert 0.05 * wl.n < (~ok).sum() < 0.2 * wl.n
    w = gpu_worker_factory(wl.capacity)
    try:
        b = gpu.DeviceBatch(w, wl.frames, wl.desc[:n])
        for rings, rr in ((2, 1), (64, 61)):
            got = _dispatch(w, b, n, rings, rr)
            _check(got, hashes[:n], ok[:n], wl.desc[:n], rings, rr, f"n {n} rings {rings}")
        # the optional outputs left out: the required ones are the same
        got = _dispatch(w, b, n, 4, 2, flow_hash=False, desc_out=False)
        ring, index, counts, _ = rx.dispatch_host(hashes[:n], ok[:n], 4, 2)
        assert np.array_equal(got["ring"], ring) and np.array_equal(got["index"], index)
        assert np.array_equal(got["counts"], counts)
        b.free()
    finally:
        w.close()


def _batch(pairs):
    """(frame bytes, len) pairs -> (frames, desc)."""
    h = np.zeros((len(pairs), 128), np.uint8)
    for i, (fr, _) in enumerate(pairs):
        h[i, :len(fr)] = np.frombuffer(fr, np.uint8)
    return synth.pack_frames(h, np.array([ln for _, ln in pairs]), stride=128)


def _udp(src, dst, sp, dp):
    fr = synth._frame(synth._eth(0x0800), synth._ip4(17, src, dst), synth._udp(sp, dp))
    return fr, len(fr)


def test_pure_round_robin(gpu_worker_factory):
    """Every frame 10 bytes long: no packet parses, ring i = (rr + i) & (W - 1)."""
    n, rings, rr = B + 5, 4, 3
    frames, desc = _batch([(bytes(range(1, 11)), 10)] * n)
    w = gpu_worker_factory()
    try:
        b = gpu.DeviceBatch(w, frames, desc)
        got = _dispatch(w, b, n, rings, rr)
        b.free()
    finally:
        w.close()
    i = np.arange(n, dtype=np.uint32)
    assert np.array_equal(got["ring"], ((rr + i) & (rings - 1)) | np.uint32(rx.FALLBACK))
    _check(got, np.zeros(n, np.uint32), np.zeros(n, bool), desc, rings, rr)
    assert int(got["counts"][rings]) == n


def test_one_flow(gpu_worker_factory):
    """One flow repeated B + 5 times: its ring holds everything, the others nothing."""
    n, rings = B + 5, 64
    fr = _udp(0x0A000001, 0x0A800007, 1234, 53)
    rc, key = oracle.parse(fr[0], fr[1])
    assert rc == 0
    h = int(oracle.oracle_lib().upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p)))
    frames, desc = _batch([fr] * n)
    w = gpu_worker_factory()
    try:
        b = gpu.DeviceBatch(w, frames, desc)
        got = _dispatch(w, b, n, rings, 5)
        b.free()
    finally:
        w.close()
    want = np.zeros(rings + 1, np.uint64)
    want[h & (rings - 1)] = n
    assert np.array_equal(got["counts"], want)
    assert np.all(got["ring"] == (h & (rings - 1)))
    assert np.array_equal(got["index"], np.arange(n, dtype=np.uint32))
    assert np.all(got["flow_hash"] == h)


def test_parsed_packet_with_hash_zero(gpu_worker_factory):
    """UDP with src = dst, sport 17, dport 0 hashes to 0 and parsed: ring 0 without the fallback
    bit, and the cursor stays where it was."""
    zero = _udp(0x0A000001, 0x0A000001, 17, 0)
    rc, key = oracle.parse(zero[0], zero[1])
    assert rc == 0
    assert oracle.oracle_lib().upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p)) == 0
    short = (bytes(10), 10)
    frames, desc = _batch([short, zero, short])
    w = gpu_worker_factory()
    try:
        b = gpu.DeviceBatch(w, frames, desc)
        got = _dispatch(w, b, 3, 4, 2)
        b1 = gpu.DeviceBatch(w, *_batch([zero]))
        only = _dispatch(w, b1, 1, 4, 2)
        b1.free()
        b.free()
    finally:
        w.close()
    assert got["ring"].tolist() == [2 | rx.FALLBACK, 0, 3 | rx.FALLBACK]
    assert got["counts"].tolist() == [1, 0, 1, 1, 2]
    assert got["index"].tolist() == [1, 0, 2]
    assert only["ring"].tolist() == [0] and only["counts"].tolist() == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("rings", [4, 64])
def test_cursor_carry(gpu_worker_factory, rings):
    """config_d_small as [0, 1000) then [1000, n), the cursor taken from d_counts[rings]: the
    ring ids of the single call."""
    wl, _ = golden_io.load("config_d_small")
    cut, rr = 1000, 3
    w = gpu_worker_factory(wl.capacity)
    try:
        whole = gpu.DeviceBatch(w, wl.frames, wl.desc)
        head = gpu.DeviceBatch(w, wl.frames, wl.desc[:cut])
        tail = gpu.DeviceBatch(w, wl.frames, wl.desc[cut:])
        one = _dispatch(w, whole, wl.n, rings, rr)
        a = _dispatch(w, head, cut, rings, rr)
        rr2 = (rr + int(a["counts"][rings])) & (rings - 1)
        c = _dispatch(w, tail, wl.n - cut, rings, rr2)
        for x in (whole, head, tail):
            x.free()
    finally:
        w.close()
    assert int(a["counts"][rings]) > 0 and int(c["counts"][rings]) > 0
    assert np.array_equal(np.concatenate([a["ring"], c["ring"]]), one["ring"])
    assert np.array_equal(a["counts"] + c["counts"], one["counts"])


@pytest.mark.parametrize("rings", [2, 4])
@pytest.mark.parametrize("case", ["config_b_small", "config_c_small", "config_d_small"])
def test_workers_fed_by_the_dispatch(gpu_worker_factory, case, rings):
    """The reference's deployment (src/main.c:444-456): the batch dispatched, then one context
    per ring, configured from the workload, runs upe_gpu_process on its d_desc_out segment over
    the shared frames.  Verdicts, rewritten bytes, counters, rule_stats and the final L1 of each
    equal one reference worker fed that ring's packets in RX order."""
    wl, _ = golden_io.load(case)
    n = wl.n
    rx_w = gpu_worker_factory(wl.capacity)
    workers = []
    try:
        b = gpu.DeviceBatch(rx_w, wl.frames, wl.desc)
        o = Out(rx_w, n, rings)
        rx_w.rx_dispatch(b.frames, b.desc, n, rings, 0, o.ring, o.index, o.counts,
                         flow_hash=o.flow_hash, desc_out=o.desc_out)
        got = o.fetch()
        lists = rx.ring_lists(got["index"], got["counts"], rings)
        start, results = 0, []
        for r in range(rings):
            k = len(lists[r])
            assert k > 0
            w = gpu_worker_factory(wl.capacity)
            workers.append(w)
            w.configure(wl)
            verdict = w.malloc(4 * k)
            w.process(b.frames, o.desc_out + 8 * start, verdict, k)
            v = np.zeros(k, np.uint32)
            w.sync()
            w.d2h(v, verdict)
            w.sync()
            w.free(verdict)
            results.append((v,) + w.get_stats() + (w.get_l1(),))
            start += k
        frames, _ = b.fetch()
        o.free()
        b.free()
    finally:
        for w in workers:
            w.close()
        rx_w.close()
    assert start == n
    want_frames = wl.frames.copy()
    for r in range(rings):
        part = dataclasses.replace(wl, desc=wl.desc[lists[r]])
        ref = oracle.run_reference(part) if oracle.ref_available() else oracle.run_restated(part)
        v, counters, stats, l1 = results[r]
        what = f"{case} ring {r} of {rings}"
        bad = np.nonzero(v != ref.verdict)[0]
        assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first {bad[:8].tolist()}"
        assert counters.tobytes() == np.asarray(ref.counters).tobytes(), f"{what}: counters"
        assert np.array_equal(stats, ref.rule_stats), f"{what}: rule_stats"
        assert l1.tobytes() == np.asarray(ref.l1).tobytes(), f"{what}: L1 state"
        changed = ref.frames != wl.frames   # a reference worker touches its own packets only
        want_frames[changed] = ref.frames[changed]
    assert np.array_equal(frames, want_frames), "rewritten bytes differ"


@pytest.mark.parametrize("rings", [0, 3, 128])
def test_bad_rings(gpu_worker_factory, rings):
    _bad_call(gpu_worker_factory, rings=rings)


def test_null_index(gpu_worker_factory):
    _bad_call(gpu_worker_factory, rings=4, null_index=True)


def _bad_call(gpu_worker_factory, rings, null_index=False):
    """-1 with a message and no launch (every output keeps its poison); a valid call after it
    still passes."""
    wl, _ = golden_io.load("edge_zero")
    hashes, ok = golden_io.flow_hash("edge_zero")
    w = gpu_worker_factory(wl.capacity)
    try:
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        o = Out(w, wl.n, 128)
        with pytest.raises(gpu.UpeGpuError) as e:
            w.rx_dispatch(b.frames, b.desc, wl.n, rings, 0, o.ring, 0 if null_index else o.index,
                          o.counts, flow_hash=o.flow_hash, desc_out=o.desc_out)
        assert str(e.value).split(":", 1)[1].strip()
        left = o.fetch()
        for k in ("ring", "index", "flow_hash", "desc_out", "counts"):
            assert np.all(left[k].view(np.uint8) == 0xA5), f"{k} was written"
        o.free()
        got = _dispatch(w, b, wl.n, 4, 1)
        _check(got, hashes, ok, wl.desc, 4, 1)
        b.free()
    finally:
        w.close()

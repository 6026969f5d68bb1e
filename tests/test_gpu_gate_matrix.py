"""GPU: the gate matrix (tests/gates.py) through every device parser.

The device has one definition of parse_flow_key's gates (parse_key, csrc/upe_parse.h, which
upe_parse_keys calls) and three written-out statements of it: rx_parse, upe_classify's fast
path, and the L4 gate of general_path, which takes its L4 words from the header's selector (a
select chain in the scan / tree kernels, a barrel shift in the tuple-space kernels); plus
upe_ctrl_mark / upe_ctrl_gather.  All load whole 16-byte quads and model a zero-filled pktbuf by
masking, or use no byte that a length test has not covered.  Every other batch of the suite has
zeros behind each frame, where a gate that forgot its length test still answers right.  Here the
slots are filled with 0xFF, the shape's own untruncated bytes or random bytes, every shape
appears at every length, and the expected value is always the restated oracle on the same
poisoned buffer (tests/test_gate_matrix.py shows that it cannot see the fill).  The frame
comparison covers the whole buffer, so every byte at or past a frame's len must still hold its
fill afterwards.

One test places the frames at byte offsets around and above 2^32 (include/upe_gpu.h allows
offsets below 2^36) and compares every consumer's output with the same call at offsets from 0."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

import gates
import oracle
from test_gate_matrix import hashes_of
from test_gpu_parity import _assert_same
from test_gpu_rx_dispatch import Out as RxOut, _check as _rx_check
from upe_amd import gpu, rx, synth
from upe_amd.layout import EGRESS_INFO_DTYPE, V_FWD, desc_lens, desc_offsets, make_desc

pytestmark = pytest.mark.gpu

# the three fills that are not the suite's status quo, as generated; the adversarial one shuffled
CASES = [("ones", "grouped"), ("parent", "grouped"), ("random", "grouped"), ("parent", "shuffled")]
IDS = [f"{f}-{o}" for f, o in CASES]
MODES = ["scan", "tree", "tree-memory", "tss", "tss-unstaged", "small"]
KEEP = ["ip", "mac", "valid"]


@functools.lru_cache(maxsize=None)
def _matrix(fill, order, small=False):
    m = gates.matrix(fill, order)
    if small:   # the 10-rule table: the small-table kernel (kScan 0)
        m = (dataclasses.replace(m[0], rules=synth.edge_rules(), capacity=64),) + m[1:]
    m[0].frames.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _expected(fill, order, small=False):
    r = oracle.run_restated(_matrix(fill, order, small)[0], apply_control=False)
    return {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
            "rule_stats": r.rule_stats, "l1": r.l1}


@functools.lru_cache(maxsize=None)
def _hashes(fill, order):
    return hashes_of(_matrix(fill, order)[0])


def _check_verdicts(verdict, want, m, fill, what):
    wl, parent, sid, _ = m
    bad = np.nonzero(verdict != want)[0]
    assert bad.size == 0, (
        f"{what}, fill {fill}: {bad.size} verdicts differ; " +
        "; ".join(f"{gates.describe(i, wl, parent, sid)} gpu {int(verdict[i]):#x} "
                  f"oracle {int(want[i]):#x}" for i in bad[:6]))


def _check_frames(frames, want, m, fill, what):
    wl, parent, sid, _ = m
    bad = np.nonzero(frames != want)[0]
    if bad.size:
        i = min(int(bad[0]) // gates.STRIDE, wl.n - 1)
        b = int(bad[0]) - i * gates.STRIDE
        raise AssertionError(
            f"{what}, fill {fill}: {bad.size} frame bytes differ, first at byte {b} of "
            f"{gates.describe(i, wl, parent, sid)}: gpu {int(frames[bad[0]]):#x} oracle "
            f"{int(want[bad[0]]):#x} (a byte at or past len must keep its fill)")


def _check_all(got, ref, m, fill, what):
    _check_verdicts(got[1], ref["verdict"], m, fill, what)
    _check_frames(got[0], ref["frames"], m, fill, what)
    _assert_same(got, ref, f"{what}, fill {fill}")


def _set_mode(monkeypatch, mode):
    monkeypatch.setenv("UPE_GPU_TSS", "1" if mode.startswith("tss") else "0")
    monkeypatch.setenv("UPE_GPU_TREE", "0" if mode in ("scan", "small") else "1")
    monkeypatch.setenv("UPE_GPU_TREE_LDS", "0" if mode == "tree-memory" else "1")
    monkeypatch.setenv("UPE_GPU_FP_STAGE", "0" if mode.endswith("unstaged") else "1")


def _default_mode(monkeypatch):
    for k in ("UPE_GPU_TSS", "UPE_GPU_TREE", "UPE_GPU_TREE_LDS", "UPE_GPU_FP_STAGE"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("emit", [False, True], ids=["inplace", "emit"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_classify_every_match_mode(gpu_worker_factory, monkeypatch, fill, order, mode, emit):
    """The matrix through the linear scan, the decision tree (image in LDS, or read from memory),
    the tuple-space index (fingerprints staged, or not) and, with a 10-rule table, the small-table
    kernel; rewritten in place, or through the emit-mode records."""
    _set_mode(monkeypatch, mode)
    m = _matrix(fill, order, mode == "small")
    wl = m[0]
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        assert len(wl.rules) >= 61 or mode == "small"
        assert w.rule_index_kind() == (1 if mode.startswith("tss") else
                                       2 if mode.startswith("tree") else 0)
        got = gpu.run_workload(wl, worker=w, emit=emit)
        var = w.launch_info()["variant"]
    finally:
        w.close()
    assert bool(var & 1) == emit and bool(var & 2) == mode.startswith("tss")
    if mode.startswith("tree"):
        assert var & gpu.VAR_SCAN == gpu.VAR_TREE
    elif mode == "scan":
        assert var & gpu.VAR_SCAN in (gpu.VAR_FAM, gpu.VAR_GLB)
    else:   # the small table's LDS copy, and the tuple-space kernels, carry no scan bits
        assert var & gpu.VAR_SCAN == 0
    _check_all(got, _expected(fill, order, mode == "small"), m, fill, f"{mode} emit={emit}")


@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_process_rss(gpu_worker_factory, monkeypatch, fill, order):
    """upe_gpu_process_rss (the non-lean kernels): the classify outputs, and flow_hash equal to
    the reference's hash of the reference's own parse, 0 where the parse fails."""
    _default_mode(monkeypatch)
    m = _matrix(fill, order)
    wl = m[0]
    hashes, ok = _hashes(fill, order)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        fh = w.malloc(4 * wl.n)
        w.process_rss(b.frames, b.desc, b.verdict, fh, wl.n)
        frames, verdict = b.fetch()
        got_fh = np.zeros(wl.n, np.uint32)
        w.d2h(got_fh, fh)
        w.sync()
        var = w.launch_info()["variant"]
        w.free(fh)
        b.free()
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    assert var & 4 == 0, "process_rss ran a lean kernel"
    _check_all((frames, verdict, counters, stats, l1), _expected(fill, order), m, fill, "rss")
    _check_verdicts(got_fh, np.where(ok, hashes, 0).astype(np.uint32), m, fill, "rss flow_hash")


@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_process_emit_tx(gpu_worker_factory, monkeypatch, fill, order):
    """upe_gpu_process_emit_tx: the groups' list, concatenated, equals upe_gpu_compact(V_FWD) and
    the oracle's forwarded indexes; the records applied give the oracle's frames."""
    _default_mode(monkeypatch)
    m = _matrix(fill, order)
    wl, n = m[0], m[0].n
    ref = _expected(fill, order)
    groups = (n + 63) // 64
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.hdr = w.malloc(16 * n)
        tx, cnt = w.malloc(4 * n), w.malloc(4 * groups)
        idx, k = w.malloc(4 * n), w.malloc(8)
        w.process_emit_tx(b.frames, b.desc, b.verdict, b.hdr, tx, cnt, n)
        assert w.launch_info()["variant"] & gpu.VAR_TX == gpu.VAR_TX
        w.compact(b.verdict, n, V_FWD, idx, k)
        frames, verdict = b.fetch()
        rec = b.fetch_hdr()
        got_tx, got_cnt = np.zeros(n, np.uint32), np.zeros(groups, np.uint32)
        got_idx, got_k = np.zeros(n, np.uint32), np.zeros(1, np.uint64)
        for host, dev in ((got_tx, tx), (got_cnt, cnt), (got_idx, idx), (got_k, k)):
            w.d2h(host, dev)
        w.sync()
        for p in (tx, cnt, idx, k):
            w.free(p)
        b.free()
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    frames = gpu.hdr_apply(frames, wl.desc, rec)
    _check_all((frames, verdict, counters, stats, l1), ref, m, fill, "emit_tx")
    fwd = np.nonzero((ref["verdict"] & 0xF) == V_FWD)[0]
    lst = np.concatenate([got_tx[64 * g:64 * g + int(got_cnt[g])] for g in range(groups)])
    assert fwd.size > 100
    assert np.array_equal(lst.astype(np.int64), fwd), "the groups' list"
    assert int(got_k[0]) == fwd.size and np.array_equal(got_idx[:fwd.size].astype(np.int64), fwd)


@pytest.mark.parametrize("emit", [False, True], ids=["inplace", "emit"])
@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_process_mapped(gpu_worker_factory, monkeypatch, fill, order, emit):
    """upe_gpu_process_mapped[_emit] on a pinned copy: the batch classified where it lies in host
    memory."""
    _default_mode(monkeypatch)
    m = _matrix(fill, order)
    wl, n = m[0], m[0].n
    hold = [gpu.PinnedArray(wl.frames.shape, np.uint8), gpu.PinnedArray(wl.desc.shape, np.uint64),
            gpu.PinnedArray((n,), np.uint32), gpu.PinnedArray((n, 16), np.uint8)]
    w = gpu_worker_factory(wl.capacity)
    try:
        f, d, v, h = (x.array for x in hold)
        f[:], d[:], v[:], h[:] = wl.frames, wl.desc, 0, 0xEE
        w.configure(wl)
        if emit:
            w.process_mapped_emit(f, d, v, h)
        else:
            w.process_mapped(f, d, v)
        w.sync()
        assert w.launch_info()["variant"] & gpu.VAR_HOST
        frames, verdict = f.copy(), v.copy()
        if emit:
            frames = gpu.hdr_apply(frames, wl.desc, gpu.expand_records(h.copy(), verdict))
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
        for x in hold:
            x.free()
    _check_all((frames, verdict, counters, stats, l1), _expected(fill, order), m, fill,
               f"mapped emit={emit}")


@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_process_host_chunked(gpu_worker_factory, monkeypatch, fill, order):
    """upe_gpu_process_host in chunks of 333 packets: the copy-back length arithmetic must leave
    the host buffer's tails intact.  (UPE_VF_L1_INIT is relative to each chunk's start.)"""
    _default_mode(monkeypatch)
    m = _matrix(fill, order)
    wl = m[0]
    ref = _expected(fill, order)
    frames, verdict = wl.frames.copy(), np.zeros(wl.n, np.uint32)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        w.process_host(frames, wl.desc.copy(), verdict, 333)
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    init = np.uint32(0x80)
    _check_verdicts(verdict & ~init, ref["verdict"] & ~init, m, fill, "host chunk 333")
    _check_frames(frames, ref["frames"], m, fill, "host chunk 333")
    _assert_same((frames, verdict, counters, stats, l1), ref, f"host chunk 333, fill {fill}",
                 batch_relative=True)


@pytest.mark.parametrize("rings", [4, 64])
@pytest.mark.parametrize("fill,order", CASES, ids=IDS)
def test_rx_dispatch(gpu_worker_factory, fill, order, rings):
    """upe_gpu_rx_dispatch (rx_parse): ring, index, counts, flow_hash and desc_out against
    rx.dispatch_host over the reference's parse; the frames byte-identical afterwards."""
    m = _matrix(fill, order)
    wl = m[0]
    hashes, ok = _hashes(fill, order)
    w = gpu_worker_factory(wl.capacity)
    try:
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        o = RxOut(w, wl.n, rings)
        try:
            w.rx_dispatch(b.frames, b.desc, wl.n, rings, 3, o.ring, o.index, o.counts,
                          flow_hash=o.flow_hash, desc_out=o.desc_out)
            got = o.fetch()
        finally:
            o.free()
        frames, _ = b.fetch()
        b.free()
    finally:
        w.close()
    want = np.where(ok, hashes & np.uint32(rings - 1), np.uint32(0xFFFFFFFF))
    _check_verdicts(np.where(got["ring"] & rx.FALLBACK, np.uint32(0xFFFFFFFF), got["ring"]),
                    want, m, fill, f"rx ring ids (0xffffffff: fallback), rings {rings}")
    _rx_check(got, hashes, ok, wl.desc, rings, 3, f"fill {fill} rings {rings}")
    assert np.array_equal(frames, wl.frames), "the dispatch wrote to the frames"


@functools.lru_cache(maxsize=None)
def _control(fill):
    m = gates.control_subset(fill)
    return m, oracle.run_restated(m[0], apply_control=True)


def _table_writes(wl, verdict):
    """The calls of arp_update / ndp_update handle_control_packet makes over the batch
    (src/worker.c:30-39, 64-95; oracle/cpu_ref.c control_packet): one per well-formed ARP packet,
    and one per consumed NS / NA whose option walk, over the frame's first len bytes, reaches an
    SLLA / TLLA option that lies below len."""
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    writes = int(np.count_nonzero(verdict & 0x20))
    for i in np.nonzero((verdict & 0xF) == 5)[0]:
        d, ln, off = wl.frames[offs[i]:offs[i] + lens[i]], int(lens[i]), 78
        while off + 2 <= ln:
            ol = (int(d[off + 1]) * 8) & 0xFF
            if ol == 0 or off + ol > ln:
                break
            if ol >= 8 and int(d[off]) == (1 if d[54] == 135 else 2):
                writes += 1
                break
            off += ol
    return writes


@pytest.mark.parametrize("fill", ["ones", "parent", "random"])
def test_segmented_control_subset(gpu_worker_factory, monkeypatch, fill):
    """upe_gpu_process_segmented (upe_ctrl_mark / upe_ctrl_gather and the host's option walk):
    every truncation of every ARP / NS / NA shape, each followed by probes to the address the
    whole frame teaches.  Under the `parent` fill an NS cut inside its option has the option's
    MAC lying past len; the oracle's zero-filled buffer decides what is learned."""
    _default_mode(monkeypatch)
    m, r = _control(fill)
    wl = m[0]
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        arp, ndp = wl.arp.copy(), wl.ndp.copy()
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        writes = w.process_segmented(b.frames, b.desc, b.verdict, b.n, arp, ndp, now=1234)
        frames, verdict = b.fetch()
        b.free()
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    init = np.uint32(0x80)   # relative to each segment's start
    _check_verdicts(verdict & ~init, r.verdict & ~init, m, fill, "segmented")
    _check_frames(frames, r.frames, m, fill, "segmented")
    _assert_same((frames, verdict, counters, stats, l1),
                 {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
                  "rule_stats": r.rule_stats, "l1": r.l1}, f"segmented, fill {fill}",
                 batch_relative=True)
    assert np.array_equal(arp[KEEP], r.arp[KEEP]), f"fill {fill}: final ARP table"
    assert np.array_equal(ndp[KEEP], r.ndp[KEEP]), f"fill {fill}: final NDP table"
    assert not np.array_equal(arp[KEEP], wl.arp[KEEP]) and not np.array_equal(ndp[KEEP], wl.ndp[KEEP])
    assert writes == _table_writes(wl, r.verdict), "n_writes"


# ---------------------------------------------------------------------------------------------
# byte offsets at and above 4 GiB
# ---------------------------------------------------------------------------------------------

GIB4 = 1 << 32
BIG = GIB4 + (2 << 20)
CANARY_BYTES = 1 << 20
CANARY = 0xC5


def _fetch(w, dptr, shape, dtype):
    out = np.zeros(shape, dtype)
    if out.size:
        w.d2h(out, dptr)
        w.sync()
    return out


def _runs_at(worker_factory, wl, base, delta):
    """In place, emit, process_rss, rx_dispatch and egress_pack (after the in-place run) over
    wl's frames uploaded at base + delta, the descriptors carrying offsets from delta; every
    output in a small allocation of its own.  Returns the outputs by name."""
    n = wl.n
    desc = make_desc(desc_offsets(wl.desc) + delta, desc_lens(wl.desc))
    out = {}

    def fresh():
        w = worker_factory(wl.capacity)
        w.configure(wl)
        w.h2d(base + delta, wl.frames)
        d, v = w.malloc(8 * n), w.malloc(4 * n)
        w.h2d(d, desc)
        w.h2d(v, np.full(n, 0xA5A5A5A5, np.uint32))
        w.sync()
        return w, d, v

    def state(w, name, v):
        out[name + ".verdict"] = _fetch(w, v, n, np.uint32)
        out[name + ".frames"] = _fetch(w, base + delta, wl.frames.shape, np.uint8)
        c, s = w.get_stats()
        out[name + ".counters"], out[name + ".stats"], out[name + ".l1"] = c, s, w.get_l1()

    # in place, then the pack of what it forwarded
    w, d, v = fresh()
    try:
        w.process(base, d, v, n)
        state(w, "inplace", v)
        ob = n * gates.STRIDE
        po, pd, pi, pinfo = w.malloc(ob), w.malloc(8 * n), w.malloc(4 * n), w.malloc(32)
        for p, size in ((po, ob), (pd, 8 * n), (pi, 4 * n), (pinfo, 32)):
            w.h2d(p, np.full(size, 0xA5, np.uint8))
        w.egress_pack(base, d, v, n, po, ob, pd, pinfo, out_index=pi)
        info = w.fetch_egress_info(pinfo)
        out["pack.info"] = np.array([int(info[k]) for k in EGRESS_INFO_DTYPE.names])
        out["pack.out"] = _fetch(w, po, ob, np.uint8)
        out["pack.desc"] = _fetch(w, pd, n, np.uint64)
        out["pack.index"] = _fetch(w, pi, n, np.uint32)
        for p in (po, pd, pi, pinfo, d, v):
            w.free(p)
    finally:
        w.close()
    # emit
    w, d, v = fresh()
    try:
        h = w.malloc(16 * n)
        w.h2d(h, np.full(16 * n, 0xA5, np.uint8))
        w.process_emit(base, d, v, h, n)
        w.sync()
        state(w, "emit", v)
        out["emit.records"] = gpu.expand_records(_fetch(w, h, (n, 16), np.uint8),
                                                 out["emit.verdict"])
        for p in (h, d, v):
            w.free(p)
    finally:
        w.close()
    # rss
    w, d, v = fresh()
    try:
        fh = w.malloc(4 * n)
        w.process_rss(base, d, v, fh, n)
        w.sync()
        state(w, "rss", v)
        out["rss.flow_hash"] = _fetch(w, fh, n, np.uint32)
        for p in (fh, d, v):
            w.free(p)
    finally:
        w.close()
    # rx dispatch
    w, d, v = fresh()
    try:
        o = RxOut(w, n, 4)
        try:
            w.rx_dispatch(base, d, n, 4, 3, o.ring, o.index, o.counts, flow_hash=o.flow_hash,
                          desc_out=o.desc_out)
            got = o.fetch()
        finally:
            o.free()
        for k, x in got.items():
            out["rx." + k] = x
        # desc_out through the offsets
        out["rx.desc_out"] = got["desc_out"] - (np.uint64(delta) << np.uint64(16))
        out["rx.frames"] = _fetch(w, base + delta, wl.frames.shape, np.uint8)
        for p in (d, v):
            w.free(p)
    finally:
        w.close()
    return out


def test_offsets_at_and_above_4gib(gpu_worker_factory, monkeypatch):
    """The boundary subset (frames within a byte of a gate, `parent` fill) in one allocation of
    4 GiB + 2 MiB, its slots straddling byte 2^32 (the first starts at 2^32 - 512): classify in
    place and in emit mode, process_rss, rx_dispatch and egress_pack give what they give for the
    same frames at offsets from 0, and the first MiB of the allocation (where an offset cut to
    32 bits would land) keeps its canary.  Under 1 MiB of the allocation is touched."""
    _default_mode(monkeypatch)
    m = gates.boundary_subset("parent")
    wl, parent, sid, _ = m
    assert wl.n <= gates.MAX_SUBSET
    delta = GIB4 - 2 * gates.STRIDE
    assert delta % 16 == 0 and delta + wl.frames.nbytes < BIG and wl.frames.nbytes < CANARY_BYTES
    assert delta + wl.frames.nbytes - GIB4 > wl.frames.nbytes // 2   # most slots lie above 2^32
    r = oracle.run_restated(wl, apply_control=False)
    w0 = gpu_worker_factory(wl.capacity)
    big = low = 0
    try:
        big = w0.malloc(BIG)
        low = w0.malloc(wl.frames.nbytes)
        w0.h2d(big, np.full(CANARY_BYTES, CANARY, np.uint8))
        w0.sync()
        lo = _runs_at(gpu_worker_factory, wl, low, 0)
        hi = _runs_at(gpu_worker_factory, wl, big, delta)
        canary = _fetch(w0, big, CANARY_BYTES, np.uint8)
    finally:
        for p in (big, low):
            if p:
                w0.free(p)
        w0.close()
    # the low run is the oracle's, so the comparison below is against a trusted value
    _check_all((lo["inplace.frames"], lo["inplace.verdict"], lo["inplace.counters"],
                lo["inplace.stats"], lo["inplace.l1"]),
               {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
                "rule_stats": r.rule_stats, "l1": r.l1}, m, "parent", "offsets from 0")
    assert int(lo["pack.info"][1]) > 50, "the subset forwards too little to test the pack"
    assert np.all(canary == CANARY), \
        f"{np.count_nonzero(canary != CANARY)} canary bytes below 1 MiB were written"
    assert sorted(lo) == sorted(hi)
    for k in sorted(lo):
        if k.endswith(".verdict") or k in ("rss.flow_hash", "rx.ring"):
            _check_verdicts(hi[k], lo[k], m, "parent", f"{k}: offsets from 2^32 - 512 (as gpu) "
                            f"against offsets from 0 (as oracle)")
        elif k.endswith(".frames"):
            _check_frames(hi[k], lo[k], m, "parent", f"{k} at offsets from 2^32 - 512")
        else:
            assert np.asarray(hi[k]).tobytes() == np.asarray(lo[k]).tobytes(), \
                f"{k} differs between offsets from 2^32 - 512 and offsets from 0"

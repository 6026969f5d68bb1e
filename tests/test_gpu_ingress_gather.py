"""GPU: upe_gpu_ingress_gather, a burst of pktbuf handles (buffer indexes into a pool of
stride-byte buffers: timestamp@0, len@8, data@16) gathered on the device into the "Batch layout"
— in place (REF), as 96-byte header windows (WINDOW) or packed back to back (FULL) — with the
buffers' timestamps, the positions of the packets that may write a neighbour table, and the
summary.  Expected values come from ingress.gather_host, which tests/test_ingress_gather.py pins
to the golden frames; end to end, from the reference's golden outputs and the oracle.  Every
comparison is bit-exact."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import golden_io
import oracle
from upe_amd import gpu, ingress
from upe_amd.layout import (FRAME_TAIL, HDR_WINDOW, INGRESS_INFO_DTYPE, desc_lens, desc_offsets)

pytestmark = pytest.mark.gpu

B = gpu.INGRESS_BLOCK   # packets per workgroup of the gather kernels
LENS = np.array([0, 1, 13, 14, 15, 16, 17, 59, 60, 64, 77, 78, 95, 96, 97, 128, 1514, 2048])
SIZES = [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17]
STRIDES = [2064, 128, 4112]
MODES = {"ref": ingress.REF, "window": ingress.WINDOW, "full": ingress.FULL}
CANARY = 4096
POISON = 0xA5
NONE = 2**64 - 1
INFO_FIELDS = INGRESS_INFO_DTYPE.names


@functools.lru_cache(maxsize=4)
def _random_pool(n, stride):
    """2n buffers of random bytes (so the data past every len is stale garbage) with random
    timestamps and lengths drawn from LENS, capped at stride - 16."""
    rng = np.random.default_rng(100 * n + stride)
    cap = 2 * n
    pool = rng.integers(0, 256, (cap, stride), dtype=np.uint8)
    head = np.zeros((cap, 2), "<u8")
    head[:, 0] = rng.integers(0, 1 << 63, cap, dtype=np.uint64)
    head[:, 1] = np.minimum(rng.choice(LENS, cap), stride - 16)
    head[0, 1], head[cap - 1, 1] = min(2048, stride - 16), 17
    pool[:, :16] = head.view(np.uint8)
    pool = pool.reshape(-1)
    pool.setflags(write=False)
    return pool


def _slot_patterns(n):
    rng = np.random.default_rng(3 * n + 2)
    return {
        "identity": np.arange(n),
        "reversed": np.arange(n)[::-1],
        "permutation": rng.permutation(2 * n)[:n],
        "twice": np.repeat(np.arange((n + 1) // 2), 2)[:n],
        "same": np.full(n, n - 1),
    }


class Outs:
    """Device outputs of one gather, each with CANARY bytes behind it, everything poisoned."""

    def __init__(self, w, n, out_bytes, opt=True, out=True):
        self.w, self.n, self.out_bytes = w, n, out_bytes
        self.sizes = {"out": out_bytes if out else None, "desc": 8 * n,
                      "ts": 8 * n if opt else None, "ctrl": 4 * n if opt else None, "info": 64}
        self.p = {}
        for k, size in self.sizes.items():
            self.p[k] = 0
            if size is not None:
                self.p[k] = w.malloc(size + CANARY)
                w.h2d(self.p[k], np.full(size + CANARY, POISON, np.uint8))
        w.sync()

    def gather(self, pool, pool_bytes, stride, slot, mode, n=None, **over):
        a = {"out": self.p["out"] or None, "out_bytes": self.out_bytes if self.p["out"] else 0,
             "desc": self.p["desc"], "info": self.p["info"], "timestamp": self.p["ts"] or None,
             "ctrl": self.p["ctrl"] or None}
        a.update(over)
        self.w.ingress_gather(pool, pool_bytes, stride, slot, self.n if n is None else n, mode,
                              a["desc"], a["info"], out=a["out"], out_bytes=a["out_bytes"],
                              timestamp=a["timestamp"], ctrl=a["ctrl"])

    def fetch(self):
        self.w.sync()
        got = {}
        for k, size in self.sizes.items():
            if size is not None:
                got[k] = np.zeros(size + CANARY, np.uint8)
                self.w.d2h(got[k], self.p[k])
        self.w.sync()
        return got

    def free(self):
        for p in self.p.values():
            if p:
                self.w.free(p)


def _untouched(got):
    return all(np.all(a == POISON) for a in got.values())


def _check(got, want, n, what):
    """Everything the contract defines against gather_host's, and the poison everywhere else."""
    out, desc, ts, ctrl, info = want
    gi = got["info"][:64].view(INGRESS_INFO_DTYPE)[0]
    assert tuple(int(gi[k]) for k in INFO_FIELDS) == tuple(int(info[k]) for k in INFO_FIELDS), \
        f"{what}: info {gi} want {info}"
    assert np.all(got["info"][64:] == POISON), f"{what}: canary behind info"
    used, packed = int(info["bytes"]), int(info["packed"])
    if "out" in got:
        bad = np.nonzero(got["out"][:used] != out)[0]
        assert bad.size == 0, (f"{what}: {bad.size} output bytes differ, first at "
                               f"{bad[:8].tolist()}: gpu {got['out'][bad[:8]].tolist()} "
                               f"want {out[bad[:8]].tolist()}")
        assert np.all(got["out"][used:] == POISON), f"{what}: bytes at or past info.bytes = {used}"
    else:
        assert used == 0
    for k, w, size in (("desc", desc, 8), ("ts", ts, 8), ("ctrl", ctrl, 4)):
        if k not in got:
            continue
        m = size * len(w)
        assert len(w) == (int(np.count_nonzero(ctrl < packed)) if k == "ctrl" else packed)
        assert got[k][:m].tobytes() == w.tobytes(), f"{what}: {k}"
        assert np.all(got[k][m:] == POISON), f"{what}: {k} from entry {len(w)} on"


def _upload(w, a):
    p = w.malloc(max(a.nbytes, 16))
    if a.nbytes:
        w.h2d(p, np.ascontiguousarray(a))
    w.sync()
    return p


def _room(want, mode, n):
    return {ingress.REF: 0, ingress.WINDOW: n * HDR_WINDOW + 32,
            ingress.FULL: int(want[4]["need"]) + 32}[mode]   # a little more: stays untouched


def _run(w, d_pool, pool, stride, slots, mode, out_bytes=None, opt=True):
    n = len(slots)
    want = ingress.gather_host(pool, stride, slots, mode,
                               out_bytes if mode == ingress.FULL else None)
    room = _room(want, mode, n) if out_bytes is None else out_bytes
    d_slot = _upload(w, np.asarray(slots, np.uint32))
    o = Outs(w, n, room, opt=opt, out=mode != ingress.REF)
    try:
        o.gather(d_pool, pool.size, stride, d_slot, mode)
        return o.fetch(), want
    finally:
        o.free()
        w.free(d_slot)


def _pool_unchanged(w, d_pool, pool):
    back = np.zeros(pool.size, np.uint8)
    w.d2h(back, d_pool)
    w.sync()
    assert np.array_equal(back, pool), "the pool was written"


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", SIZES)
def test_random_pools(gpu_worker_factory, n, stride):
    pool = _random_pool(n, stride)
    w = gpu_worker_factory()
    try:
        d_pool = _upload(w, pool)
        for pname, slots in _slot_patterns(n).items():
            for mname, mode in MODES.items():
                for opt in (True, False):
                    got, want = _run(w, d_pool, pool, stride, slots, mode, opt=opt)
                    assert int(want[4]["bad"]) == 0 and int(want[4]["packed"]) == n
                    _check(got, want, n, f"n {n} stride {stride} {pname} {mname} opt {opt}")
        _pool_unchanged(w, d_pool, pool)
        w.free(d_pool)
    finally:
        w.close()


def test_full_capacity(gpu_worker_factory):
    """out_bytes too small: the written prefix, `packed`, `bytes` and `need` as gather_host gives
    them, and neither the canary nor [bytes, out_bytes) touched."""
    n, stride = 3 * B + 17, 2064
    pool = _random_pool(n, stride)
    slots = _slot_patterns(n)["permutation"]
    _, desc, _, _, info = ingress.gather_host(pool, stride, slots, ingress.FULL)
    need = int(info["need"])
    offs = desc_offsets(desc)
    ends = offs + ((desc_lens(desc) + 15) & ~15)
    k = B + 3 * 64 + 20   # a cut inside tile 1 and inside a 64-group, with 7 bytes to spare
    caps = {"need": need, "need_less_16": need - 16, "last_frame_offset": int(offs[-1]),
            "sixteen": 16, "zero": 0, "inside_tile_and_group": int(ends[k]) + 7}
    w = gpu_worker_factory()
    try:
        d_pool = _upload(w, pool)
        for name, cap in caps.items():
            got, want = _run(w, d_pool, pool, stride, slots, ingress.FULL, out_bytes=cap)
            assert int(want[4]["need"]) == need
            if name == "need":
                assert int(want[4]["packed"]) == n
            else:
                assert int(want[4]["packed"]) < n
            _check(got, want, n, f"out_bytes {name} = {cap}")
        _pool_unchanged(w, d_pool, pool)
        w.free(d_pool)
    finally:
        w.close()


@pytest.mark.parametrize("stride", [128, 131088])
def test_bad_handles(gpu_worker_factory, stride):
    """A slot one past the last buffer, len = stride - 15, len = 2^32 + 64 and (in a pool whose
    buffers could hold it) len = 65536, first, last and on both sides of a tile boundary."""
    n, cap = 2 * B + 5, 8
    rng = np.random.default_rng(stride)
    lens = [60, 64, 17, 112, stride - 15, 2**32 + 64, 65535 if stride > 65551 else 96,
            65536 if stride > 65552 else 1]
    frames = [rng.integers(0, 256, 112, dtype=np.uint8) for _ in range(cap)]
    pool = ingress.make_pool(frames, lens, range(cap), cap, stride, fill=0x3C)
    kinds = [cap, 4, 5] + ([7] if stride > 65552 else [])   # the bad slots
    slots = rng.integers(0, 4, n)
    where = [0, 1, 2, B - 2, B - 1, B, B + 1, n - 2, n - 1]
    for j, p in enumerate(where):
        slots[p] = kinds[j % len(kinds)]
    if stride > 65552:
        slots[3] = 6   # a good frame of 65535 bytes
    w = gpu_worker_factory()
    try:
        d_pool = _upload(w, pool)
        for mname, mode in MODES.items():
            got, want = _run(w, d_pool, pool, stride, slots, mode)
            info = want[4]
            assert (int(info["bad"]), int(info["first_bad"])) == (len(where), 0)
            d = want[1]
            assert not desc_lens(d)[where].any()
            if mode != ingress.WINDOW:
                assert np.all(desc_offsets(d)[where] == 16)
            _check(got, want, n, f"stride {stride} {mname}")
        _pool_unchanged(w, d_pool, pool)
        w.free(d_pool)
    finally:
        w.close()


def _control_frames():
    arp = np.zeros(64, np.uint8)
    arp[12:20] = [0x08, 0x06, 0, 1, 8, 0, 6, 4]
    arp_hlen = arp.copy()
    arp_hlen[18] = 8
    ns = np.zeros(112, np.uint8)
    ns[12:14], ns[20], ns[54] = [0x86, 0xDD], 58, 135
    na = ns.copy()
    na[54] = 136
    udp6 = ns.copy()
    udp6[20] = 17
    plain = np.zeros(64, np.uint8)
    plain[12:14] = [0x08, 0x00]
    #        frame, len, marked
    return [(arp, 64, True), (arp_hlen, 64, False), (ns, 77, False), (ns, 78, True),
            (na, 86, True), (udp6, 86, False), (arp, 13, False), (plain, 64, False)]


def test_control_marks(gpu_worker_factory):
    """ARP, ARP with a wrong hlen, NS of 77 and 78 bytes, NA, an IPv6 non-ICMPv6 frame with byte 54
    = 135 and a 13-byte frame whose stale bytes spell an ARP header, at positions 0, B - 1, B and
    n - 1 and around them; tile 2 has none, between two tiles that have some."""
    kinds = _control_frames()
    stride, n = 128, 4 * B + 17
    pool = ingress.make_pool([k[0] for k in kinds], [k[1] for k in kinds], range(8), 8, stride)
    slots = np.full(n, 7)
    marked = [0, 3, 4]
    anchors = [0, B - 1, B, n - 1]
    for j, p in enumerate(anchors):
        slots[p] = marked[j % 3]
    for base in (1, B - 9, B + 1, 3 * B + 100, n - 9):
        slots[base:base + 8] = np.arange(8)
    assert np.all(slots[2 * B:3 * B] == 7)
    expect = np.nonzero(np.array([k[2] for k in kinds])[slots])[0]
    assert set(anchors) <= set(expect.tolist())
    w = gpu_worker_factory()
    try:
        d_pool = _upload(w, pool)
        for mname, mode in MODES.items():
            for opt in (True, False):
                got, want = _run(w, d_pool, pool, stride, slots, mode, opt=opt)
                assert np.array_equal(want[3], expect)
                assert int(want[4]["n_ctrl"]) == expect.size and int(want[4]["first_ctrl"]) == 0
                _check(got, want, n, f"control marks {mname} opt {opt}")
        # a cut in FULL mode: the counts cover all n, the list stops at `packed`
        cap = int(desc_offsets(want[1])[B + 4])
        got, want = _run(w, d_pool, pool, stride, slots, ingress.FULL, out_bytes=cap)
        assert 0 < len(want[3]) < expect.size == int(want[4]["n_ctrl"])
        _check(got, want, n, "control marks with a cut")
        w.free(d_pool)
    finally:
        w.close()


def test_offsets_past_4gib(gpu_worker_factory):
    """A pool of 4 GiB + 8 buffers in device memory, allocated but not filled: only the top eight
    slots are written and gathered, in all three modes."""
    stride = 2064
    pool_bytes = (1 << 32) + 8 * stride
    nbuf = pool_bytes // stride
    top = nbuf - 8
    assert top * stride < 1 << 32 < (nbuf - 7) * stride   # all but the first start past 4 GiB
    rng = np.random.default_rng(8)
    mini = rng.integers(0, 256, (8, stride), dtype=np.uint8)
    head = np.zeros((8, 2), "<u8")
    head[:, 0] = rng.integers(0, 1 << 63, 8, dtype=np.uint64)
    head[:, 1] = [2048, 0, 17, 64, 1514, 96, 78, 1]
    mini[:, :16] = head.view(np.uint8)
    mini = mini.reshape(-1)
    order = np.array([7, 0, 3, 3, 5, 1, 6, 2, 4])
    w = gpu_worker_factory()
    try:
        d_pool = w.malloc(pool_bytes)
        w.h2d(d_pool + top * stride, mini)
        d_slot = _upload(w, (order + top).astype(np.uint32))
        for mname, mode in MODES.items():
            out, desc, ts, ctrl, info = ingress.gather_host(mini, stride, order, mode)
            if mode == ingress.REF:
                desc = desc + (np.uint64(top * stride) << np.uint64(16))
            want = (out, desc, ts, ctrl, info)
            o = Outs(w, len(order), _room(want, mode, len(order)), out=mode != ingress.REF)
            o.gather(d_pool, pool_bytes, stride, d_slot, mode)
            got = o.fetch()
            o.free()
            _check(got, want, len(order), f"past 4 GiB {mname}")
        # one past the top is outside
        w.h2d(d_slot, np.array([nbuf, nbuf - 1], np.uint32))
        o = Outs(w, 2, 0, out=False)
        o.gather(d_pool, pool_bytes, stride, d_slot, ingress.REF)
        gi = o.fetch()["info"][:64].view(INGRESS_INFO_DTYPE)[0]
        o.free()
        assert (int(gi["bad"]), int(gi["first_bad"])) == (1, 0)
        w.free(d_slot)
        w.free(d_pool)
    finally:
        w.close()


# ---- end to end ------------------------------------------------------------------------------

E2E = ["config_a", "config_c_small", "edge_zero", "edge_consistent", "ndp_walk"]


@functools.lru_cache(maxsize=None)
def _scattered(case):
    """The case's frames in a stride-2064 pool twice as large, at a random permutation of slots,
    and what one classify launch over them must give: the golden (reference) outputs, or for the
    cases with control packets the oracle's with the table writes deferred, as
    tests/test_gpu_parity.py compares a batch run as one segment."""
    wl, ref = golden_io.load(case)
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    frames = [wl.frames[o:o + ln] for o, ln in zip(offs, lens)]
    rng = np.random.default_rng(len(case) * 1000 + wl.n)
    slots = rng.permutation(2 * wl.n)[:wl.n].astype(np.uint32)
    pool = ingress.make_pool(frames, lens, slots, 2 * wl.n, 2064)
    if case not in ("config_a", "config_c_small"):
        r = oracle.run_restated(wl, apply_control=False)
        ref = {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
               "rule_stats": r.rule_stats, "l1": r.l1}
    return wl, ref, pool, slots


def _frame_bytes(buf, starts, lens):
    return [buf[s:s + ln] for s, ln in zip(starts, lens)]


@pytest.mark.parametrize("emit", [False, True], ids=["in_place", "emit"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", E2E)
def test_end_to_end(gpu_worker_factory, case, mode, emit):
    """Gather on the device, then classify what it produced: verdicts, rewritten bytes (in place,
    or the records applied by upe_hdr_apply), counters, rule_stats and L1 state are the
    reference's.  REF classifies (and rewrites) the pool itself; WINDOW is compared on the bytes a
    window holds."""
    wl, ref, pool, slots = _scattered(case)
    m = MODES[mode]
    want = ingress.gather_host(pool, 2064, slots, m)
    room = int(want[4]["bytes"]) + FRAME_TAIL
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        d_pool, d_slot = _upload(w, pool), _upload(w, slots)
        d_out = _upload(w, np.zeros(room, np.uint8)) if m != ingress.REF else 0
        d_desc, d_info = w.malloc(8 * wl.n), w.malloc(64)
        d_verdict, d_hdr = w.malloc(4 * wl.n), w.malloc(16 * wl.n)
        w.ingress_gather(d_pool, pool.size, 2064, d_slot, wl.n, m, d_desc, d_info,
                         out=d_out or None, out_bytes=room if d_out else 0)
        d_frames, size = (d_out, room) if d_out else (d_pool, pool.size)
        if emit:
            w.process_emit(d_frames, d_desc, d_verdict, d_hdr, wl.n)
        else:
            w.process(d_frames, d_desc, d_verdict, wl.n)
        w.sync()
        buf, desc = np.zeros(size, np.uint8), np.zeros(wl.n, np.uint64)
        verdict, rec = np.zeros(wl.n, np.uint32), np.zeros((wl.n, 16), np.uint8)
        for h, p in ((buf, d_frames), (desc, d_desc), (verdict, d_verdict), (rec, d_hdr)):
            w.d2h(h, p)
        info = w.fetch_ingress_info(d_info)
        counters, stats = w.get_stats()
        l1 = w.get_l1()
        for p in (d_pool, d_slot, d_out, d_desc, d_info, d_verdict, d_hdr):
            if p:
                w.free(p)
    finally:
        w.close()
    what = f"{case} {mode} {'emit' if emit else 'in place'}"
    assert info == want[4] and np.array_equal(desc, want[1]), what
    assert np.array_equal(verdict, ref["verdict"]), what
    if emit:
        buf = gpu.hdr_apply(buf, desc, gpu.expand_records(rec, verdict))
    seen = lens if m != ingress.WINDOW else np.minimum(lens, HDR_WINDOW)
    got = _frame_bytes(buf, desc_offsets(desc), seen)
    exp = _frame_bytes(ref["frames"], offs, seen)
    bad = [k for k in range(wl.n) if not np.array_equal(got[k], exp[k])]
    assert not bad, f"{what}: {len(bad)} frames differ, first {bad[:8]}"
    assert counters.tobytes() == np.asarray(ref["counters"]).tobytes(), what
    assert np.array_equal(stats, ref["rule_stats"]), what
    assert l1.tobytes() == np.asarray(ref["l1"]).tobytes(), what


def test_full_output_through_process_segmented(gpu_worker_factory):
    """ndp_walk gathered in FULL mode, then upe_gpu_process_segmented: the reference worker's
    golden outputs, table writes applied between packets."""
    wl, ref = golden_io.load("ndp_walk")
    _, _, pool, slots = _scattered("ndp_walk")
    want = ingress.gather_host(pool, 2064, slots, ingress.FULL)
    room = int(want[4]["bytes"]) + FRAME_TAIL
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        d_pool, d_slot = _upload(w, pool), _upload(w, slots)
        d_out = _upload(w, np.zeros(room, np.uint8))
        d_desc, d_info, d_verdict = w.malloc(8 * wl.n), w.malloc(64), w.malloc(4 * wl.n)
        d_ctrl = w.malloc(4 * wl.n)
        w.ingress_gather(d_pool, pool.size, 2064, d_slot, wl.n, ingress.FULL, d_desc, d_info,
                         out=d_out, out_bytes=room, ctrl=d_ctrl)
        writes = w.process_segmented(d_out, d_desc, d_verdict, wl.n, arp, ndp)
        w.sync()
        buf, verdict = np.zeros(room, np.uint8), np.zeros(wl.n, np.uint32)
        ctrl = np.zeros(wl.n, np.uint32)
        for h, p in ((buf, d_out), (verdict, d_verdict), (ctrl, d_ctrl)):
            w.d2h(h, p)
        info = w.fetch_ingress_info(d_info)
        counters, stats = w.get_stats()
        l1 = w.get_l1()
        for p in (d_pool, d_slot, d_out, d_desc, d_info, d_verdict, d_ctrl):
            w.free(p)
    finally:
        w.close()
    assert info == want[4] and int(info["n_ctrl"]) >= writes > 0
    assert np.array_equal(ctrl[:int(info["n_ctrl"])], want[3])
    assert np.array_equal(verdict & ~np.uint32(0x80), ref["verdict"] & ~np.uint32(0x80))
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    got = _frame_bytes(buf, desc_offsets(want[1]), lens)
    exp = _frame_bytes(ref["frames"], offs, lens)
    assert all(np.array_equal(a, b) for a, b in zip(got, exp)), "rewritten frames differ"
    assert counters.tobytes() == np.asarray(ref["counters"]).tobytes()
    assert np.array_equal(stats, ref["rule_stats"])
    assert l1.tobytes() == np.asarray(ref["l1"]).tobytes()
    keep = ["ip", "mac", "valid"]
    assert np.array_equal(arp[keep], ref["arp"][keep]) and np.array_equal(ndp[keep], ref["ndp"][keep])


def test_pinned_pool_ref_then_mapped_emit(gpu_worker_factory):
    """The pool in upe_gpu_host_alloc memory: REF with the descriptors written to pinned memory,
    then upe_gpu_process_mapped_emit over the pool with pinned verdicts and records."""
    wl, ref, pool, slots = _scattered("config_c_small")
    want = ingress.gather_host(pool, 2064, slots, ingress.REF)
    w = gpu_worker_factory(wl.capacity)
    pins = []
    try:
        w.configure(wl)
        for shape, dt in ((pool.size, np.uint8), (wl.n, np.uint64), (wl.n, np.uint32),
                          ((wl.n, 16), np.uint8), (wl.n, np.uint64), (1, INGRESS_INFO_DTYPE)):
            pins.append(gpu.PinnedArray(shape, dt))
        h_pool, h_desc, h_verdict, h_hdr, h_ts, h_info = pins
        h_pool.array[:] = pool
        for a in (h_desc, h_verdict, h_hdr, h_ts, h_info):
            a.array.view(np.uint8)[...] = POISON
        d_slot = _upload(w, slots)
        w.ingress_gather(h_pool.ptr, pool.size, 2064, d_slot, wl.n, ingress.REF, h_desc.ptr,
                         h_info.ptr, timestamp=h_ts.ptr)
        w.process_mapped_emit(h_pool.array, h_desc.array, h_verdict.array, h_hdr.array)
        w.sync()
        desc, verdict, ts = h_desc.array.copy(), h_verdict.array.copy(), h_ts.array.copy()
        rec, info, after = h_hdr.array.copy(), h_info.array[0].copy(), h_pool.array.copy()
        counters, stats = w.get_stats()
        w.free(d_slot)
    finally:
        for a in pins:
            a.free()
        w.close()
    assert info == want[4]
    assert np.array_equal(desc, want[1]) and np.array_equal(ts, want[2])
    assert np.array_equal(after, pool), "the pool was written"
    assert np.array_equal(verdict, ref["verdict"])
    buf = gpu.hdr_apply(after, desc, gpu.expand_records(rec, verdict))
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    got = _frame_bytes(buf, desc_offsets(desc), lens)
    exp = _frame_bytes(ref["frames"], offs, lens)
    assert all(np.array_equal(a, b) for a, b in zip(got, exp)), "records applied differ"
    assert counters.tobytes() == np.asarray(ref["counters"]).tobytes()
    assert np.array_equal(stats, ref["rule_stats"])


def test_scratch_growth(gpu_worker_factory):
    """One context, gathers of 65, 3B + 17 and 65 handles queued without a wait between them: the
    scratch is grown, then reused."""
    sizes = [65, 3 * B + 17, 65]
    w = gpu_worker_factory()
    held, outs, wants = [], [], []
    try:
        for n in sizes:
            pool = _random_pool(n, 128)
            slots = _slot_patterns(n)["permutation"]
            wants.append(ingress.gather_host(pool, 128, slots, ingress.FULL))
            held.append((_upload(w, pool), _upload(w, slots.astype(np.uint32)), pool.size))
            outs.append(Outs(w, n, int(wants[-1][4]["need"])))
        for (d_pool, d_slot, size), o in zip(held, outs):
            o.gather(d_pool, size, 128, d_slot, ingress.FULL)
        for n, o, want in zip(sizes, outs, wants):
            _check(o.fetch(), want, n, f"gather of {n} in a queue of three")
        for o in outs:
            o.free()
        for d_pool, d_slot, _ in held:
            w.free(d_pool)
            w.free(d_slot)
    finally:
        w.close()


def test_empty_burst(gpu_worker_factory):
    """n == 0 zeroes *d_info, with first_bad = first_ctrl = UINT64_MAX, and writes nothing else."""
    pool = _random_pool(1, 128)
    w = gpu_worker_factory()
    try:
        d_pool = _upload(w, pool)
        for mode in MODES.values():
            o = Outs(w, 0, 64, out=mode != ingress.REF)
            o.gather(d_pool, pool.size, 128, 0, mode)
            got = o.fetch()
            o.free()
            want = np.zeros(1, INGRESS_INFO_DTYPE)
            want["first_bad"] = want["first_ctrl"] = NONE
            assert got["info"][:64].tobytes() == want.tobytes()
            assert np.all(got["info"][64:] == POISON)
            assert all(np.all(got[k] == POISON) for k in got if k != "info")
        w.free(d_pool)
    finally:
        w.close()


ERRORS = ["null_info", "null_pool", "null_slot", "null_desc", "unknown_mode", "stride_not_16",
          "stride_too_small", "pool_smaller_than_stride", "pool_past_2_36", "pool_misaligned",
          "out_misaligned", "out_in_ref_mode", "out_missing_window", "out_missing_full",
          "window_out_too_small", "n_past_32_bits", "out_inside_pool", "pool_not_mapped"]


@pytest.mark.parametrize("how", ERRORS)
def test_bad_arguments(gpu_worker_factory, how):
    """-1 with a message and no launch (every output keeps its poison); a valid call after it
    still passes."""
    n, stride = 65, 128
    pool = _random_pool(n, stride)
    slots = _slot_patterns(n)["permutation"]
    mode = {"out_in_ref_mode": ingress.REF, "out_missing_window": ingress.WINDOW,
            "window_out_too_small": ingress.WINDOW}.get(how, ingress.FULL)
    want = ingress.gather_host(pool, stride, slots, ingress.FULL)
    room = max(int(want[4]["need"]), n * HDR_WINDOW)
    w = gpu_worker_factory()
    try:
        d_pool, d_slot = _upload(w, pool), _upload(w, slots.astype(np.uint32))
        o = Outs(w, n, room)
        a = {"pool": d_pool, "pool_bytes": pool.size, "stride": stride, "slot": d_slot, "n": n,
             "mode": mode}
        over = {}
        if how == "null_info":
            over["info"] = 0
        elif how == "null_pool":
            a["pool"] = 0
        elif how == "null_slot":
            a["slot"] = 0
        elif how == "null_desc":
            over["desc"] = 0
        elif how == "unknown_mode":
            a["mode"] = 3
        elif how == "stride_not_16":
            a["stride"] = 120
        elif how == "stride_too_small":
            a["stride"] = 96
        elif how == "pool_smaller_than_stride":
            a["pool_bytes"] = stride - 16
        elif how == "pool_past_2_36":
            a["pool_bytes"] = (1 << 36) + 16
        elif how == "pool_misaligned":
            a["pool"] = d_pool + 8
        elif how == "out_misaligned":
            over["out"] = o.p["out"] + 8
        elif how in ("out_missing_window", "out_missing_full"):
            over["out"], over["out_bytes"] = None, 0
        elif how == "window_out_too_small":
            over["out_bytes"] = n * HDR_WINDOW - 1
        elif how == "n_past_32_bits":
            a["n"] = 2**32 - B
        elif how == "out_inside_pool":
            over["out"] = d_pool + 256
        elif how == "pool_not_mapped":
            host = pool.copy()   # pageable host memory: the device cannot load from it
            a["pool"] = host.ctypes.data & ~15
        with pytest.raises(gpu.UpeGpuError) as e:
            o.gather(a["pool"], a["pool_bytes"], a["stride"], a["slot"], a["mode"], n=a["n"],
                     **over)
        assert str(e.value).split(":", 1)[1].strip()
        assert _untouched(o.fetch()), "an output was written"
        _pool_unchanged(w, d_pool, pool)
        o.free()
        got, want = _run(w, d_pool, pool, stride, slots, ingress.FULL)
        _check(got, want, n, f"after {how}")
        w.free(d_pool)
        w.free(d_slot)
    finally:
        w.close()

"""GPU: upe_gpu_egress_pack, the forwarded frames of a classified batch packed back to back on the
device in the order the reference queues them for tx_send_batch (src/worker.c:240-243, 287-303),
rewritten as process_packet leaves them — copied (in-place mode) or with the emit-mode records
applied (UPE_HDR_SLOT layout).  Expected values come from egress.pack_host, which
tests/test_egress_pack.py pins to the reference's frames; end to end, from the reference's golden
frames and verdicts themselves."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

import golden_io
import oracle
from upe_amd import egress, gpu
from upe_amd.layout import EGRESS_INFO_DTYPE, FRAME_TAIL, V_FWD, desc_lens, desc_offsets

pytestmark = pytest.mark.gpu

B = gpu.EGRESS_BLOCK   # packets per workgroup of the pack kernels
LENS = np.array([42, 60, 63, 64, 65, 79, 80, 81, 128, 1514, 2048, 9000, 65535])
SIZES = [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17]
CANARY = 4096
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _synthetic(n):
    """n frames of random bytes, lengths drawn from LENS, at 16-byte aligned offsets; records with
    b[15] in {4, 6} and random other bytes in every slot; a random verdict word per packet whose
    code is not FWD (the patterns put FWD in)."""
    rng = np.random.default_rng(1000 + n)
    lens = rng.choice(LENS, n)
    lens[0], lens[-1] = (65535, 81) if n > 1 else (81, 81)
    padded = (lens + 15) & ~15
    offs = np.cumsum(padded) - padded
    frames = rng.integers(0, 256, int(padded.sum()) + FRAME_TAIL, dtype=np.uint8)
    desc = (offs.astype(np.uint64) << np.uint64(16)) | lens.astype(np.uint64)
    rec = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    rec[:, 15] = rng.choice([4, 6], n)
    other = rng.choice([0, 1, 2, 3, 5, 6], n).astype(np.uint32)
    high = rng.integers(0, 1 << 28, n, dtype=np.uint32) << np.uint32(4)   # flag and rule bits
    for a in (frames, desc, rec, other, high):
        a.setflags(write=False)
    return frames, desc, rec, other, high


def _patterns(n):
    """name -> which packets are forwarded."""
    rng = np.random.default_rng(7 * n + 1)
    i = np.arange(n)
    pats = {
        "none": np.zeros(n, bool),
        "all": np.ones(n, bool),
        "first": i == 0,
        "last": i == n - 1,
        # one forwarded packet per 64-group, at a lane that varies with the group
        "one_per_group": (i % 64) == np.minimum((i // 64 * 37 + 11) % 64, (n - 1) - (i & ~63)),
        "p50": rng.random(n) < 0.5,
        "p02": rng.random(n) < 0.02,
    }
    if n > 2 * B:   # a whole tile with nothing forwarded between two that forward
        pats["empty_tile"] = pats["p50"] & ((i < B) | (i >= 2 * B))
    return pats


def _verdict(n, fwd):
    _, _, _, other, high = _synthetic(n)
    return (np.where(fwd, np.uint32(V_FWD), other) | high).astype(np.uint32)


class Dev:
    """The ingress side of one batch on the device: frames, descriptors, records, a verdict
    array to fill."""

    def __init__(self, w, frames, desc, rec=None):
        self.w, self.n = w, len(desc)
        self.frames, self.desc = w.malloc(frames.nbytes), w.malloc(max(desc.nbytes, 8))
        self.verdict = w.malloc(max(4 * self.n, 4))
        self.rec = w.malloc(max(16 * self.n, 16)) if rec is not None else 0
        w.h2d(self.frames, np.ascontiguousarray(frames))
        if self.n:
            w.h2d(self.desc, np.ascontiguousarray(desc))
            if rec is not None:
                w.h2d(self.rec, np.ascontiguousarray(rec))
        w.sync()

    def set_verdict(self, v):
        if self.n:
            self.w.h2d(self.verdict, np.ascontiguousarray(v, np.uint32))
            self.w.sync()

    def free(self):
        for p in (self.frames, self.desc, self.verdict, self.rec):
            if p:
                self.w.free(p)


class Out:
    """Device outputs of one pack: d_out of out_bytes with CANARY bytes behind it, everything
    poisoned before the call."""

    def __init__(self, w, n, out_bytes, index=True):
        self.w, self.n, self.out_bytes = w, n, out_bytes
        m = max(n, 1)
        self.out = w.malloc(out_bytes + CANARY)
        self.desc = w.malloc(8 * m)
        self.index = w.malloc(4 * m) if index else 0
        self.info = w.malloc(32)
        for p, size in ((self.out, out_bytes + CANARY), (self.desc, 8 * m), (self.index, 4 * m),
                        (self.info, 32)):
            if p:
                w.h2d(p, np.full(size, POISON, np.uint8))
        w.sync()

    def fetch(self):
        w = self.w
        w.sync()
        got = {"out": np.zeros(self.out_bytes + CANARY, np.uint8),
               "desc": np.zeros(self.n, np.uint64), "index": np.zeros(self.n, np.uint32),
               "info": np.zeros(1, EGRESS_INFO_DTYPE)}
        for k, p in (("out", self.out), ("desc", self.desc), ("index", self.index),
                     ("info", self.info)):
            if p and got[k].size:
                w.d2h(got[k], p)
        w.sync()
        return got

    def free(self):
        for p in (self.out, self.desc, self.index, self.info):
            if p:
                self.w.free(p)


def _check(got, want, out_bytes, what, index=True):
    """Every output against pack_host's, and nothing written where nothing belongs."""
    out, out_desc, out_index, info = want
    gi = got["info"][0]
    assert tuple(int(gi[k]) for k in ("frames", "packed", "bytes", "need")) == \
        tuple(int(info[k]) for k in ("frames", "packed", "bytes", "need")), f"{what}: info {gi}"
    used, packed = int(info["bytes"]), int(info["packed"])
    assert used <= out_bytes
    bad = np.nonzero(got["out"][:used] != out)[0]
    assert bad.size == 0, (f"{what}: {bad.size} packed bytes differ, first at {bad[:8].tolist()}: "
                           f"gpu {got['out'][bad[:8]].tolist()} want {out[bad[:8]].tolist()}")
    assert np.all(got["out"][used:] == POISON), \
        f"{what}: bytes at or past info.bytes = {used} were written (out_bytes {out_bytes})"
    assert np.array_equal(got["desc"][:packed], out_desc), f"{what}: out_desc"
    assert np.all(got["desc"][packed:].view(np.uint8) == POISON), f"{what}: out_desc past packed"
    if index:
        assert np.array_equal(got["index"][:packed], out_index), f"{what}: out_index"
        assert np.all(got["index"][packed:].view(np.uint8) == POISON), \
            f"{what}: out_index past packed"


def _pack(w, d, n, hdr, out_bytes, index=True):
    o = Out(w, n, out_bytes, index=index)
    try:
        w.egress_pack(d.frames, d.desc, d.verdict, n, o.out, out_bytes, o.desc, o.info,
                      hdr=d.rec if hdr else None, out_index=o.index or None)
        return o.fetch()
    finally:
        o.free()


@pytest.mark.parametrize("n", SIZES)
def test_synthetic_batches(gpu_worker_factory, n):
    frames, desc, rec, _, _ = _synthetic(n)
    w = gpu_worker_factory()
    try:
        d = Dev(w, frames, desc, rec)
        for name, fwd in _patterns(n).items():
            v = _verdict(n, fwd)
            d.set_verdict(v)
            for hdr in (False, True):
                want = egress.pack_host(frames, desc, v, hdr=rec if hdr else None)
                assert int(want[3]["frames"]) == int(np.count_nonzero(fwd))
                room = int(want[3]["need"]) + 32   # a little more than needed: stays untouched
                got = _pack(w, d, n, hdr, room)
                _check(got, want, room, f"n {n} {name} {'hdr' if hdr else 'in place'}")
        # the optional index left out: the other outputs are the same
        got = _pack(w, d, n, True, room, index=False)
        _check(got, want, room, f"n {n} without out_index", index=False)
        d.free()
    finally:
        w.close()


def test_capacity(gpu_worker_factory):
    """out_bytes too small: the packed prefix, `packed`, `bytes` and `need` as pack_host gives
    them, and neither the canary nor [bytes, out_bytes) touched.  Ordinary bounded calls."""
    n = 3 * B + 17
    frames, desc, rec, _, _ = _synthetic(n)
    v = _verdict(n, _patterns(n)["p50"])
    _, full_desc, full_index, info = egress.pack_host(frames, desc, v)
    need = int(info["need"])
    ends = desc_offsets(full_desc) + ((desc_lens(full_desc) + 15) & ~15)
    # a cut inside tile 1 and inside a 64-group: the frame of the first forwarded packet from
    # 1024 + 3 * 64 + 20 on is the last that fits, with 7 bytes to spare
    k = int(np.searchsorted(full_index, B + 3 * 64 + 20))
    assert B < full_index[k] < 2 * B and full_index[k] % 64 not in (0, 63)
    caps = {"zero": 0, "one_frame_short": need - int(ends[-1] - ends[-2]), "exact": need,
            "one_byte_short": need - 1, "inside_tile_and_group": int(ends[k]) + 7}
    w = gpu_worker_factory()
    try:
        d = Dev(w, frames, desc, rec)
        d.set_verdict(v)
        for name, cap in caps.items():
            for hdr in (False, True):
                want = egress.pack_host(frames, desc, v, hdr=rec if hdr else None, out_bytes=cap)
                assert int(want[3]["need"]) == need
                if name == "inside_tile_and_group":
                    assert int(want[3]["packed"]) == k + 1
                if name in ("one_frame_short", "one_byte_short"):
                    assert int(want[3]["packed"]) == len(ends) - 1
                got = _pack(w, d, n, hdr, cap)
                _check(got, want, cap, f"out_bytes {name} = {cap} {'hdr' if hdr else 'in place'}")
        d.free()
    finally:
        w.close()


@pytest.mark.parametrize("case", ["config_c_small", "config_cf_small"])
def test_end_to_end(gpu_worker_factory, case):
    """Classify on the device, then pack: upe_gpu_process + d_hdr = NULL, and upe_gpu_process_emit
    on a fresh copy + its records, both give the reference's forwarded frames in order; the index
    list is upe_gpu_compact's; upe_tx_flush_packed of the copied-back batch makes upe_tx_flush's
    calls from the golden."""
    wl, ref = golden_io.load(case)
    want = egress.pack_host(ref["frames"], wl.desc, ref["verdict"])
    want_tx = gpu.tx_flush(ref["frames"], wl.desc, ref["verdict"], 32)
    assert int(want[3]["frames"]) > 0
    room = int(want[3]["need"])
    for emit in (False, True):
        w = gpu_worker_factory(wl.capacity)
        try:
            w.configure(wl)
            b = gpu.DeviceBatch(w, wl.frames, wl.desc)
            if emit:
                b.run_emit()
            else:
                b.run()
            o = Out(w, wl.n, room)
            w.egress_pack(b.frames, b.desc, b.verdict, wl.n, o.out, room, o.desc, o.info,
                          hdr=b.hdr if emit else None, out_index=o.index)
            got = o.fetch()
            index, count = w.malloc(4 * wl.n), w.malloc(8)
            w.compact(b.verdict, wl.n, V_FWD, index, count)
            h_index, h_count = np.zeros(wl.n, np.uint32), np.zeros(1, np.uint64)
            w.sync()
            w.d2h(h_index, index)
            w.d2h(h_count, count)
            _, verdict = b.fetch()
            for p in (index, count):
                w.free(p)
            o.free()
            b.free()
        finally:
            w.close()
        what = f"{case} {'emit' if emit else 'in place'}"
        assert np.array_equal(verdict, ref["verdict"]), what
        _check(got, want, room, what)
        packed = int(got["info"]["packed"][0])
        assert packed == int(h_count[0])
        assert np.array_equal(got["index"][:packed], h_index[:packed]), f"{what}: compact's list"
        tx = gpu.tx_flush_packed(got["out"][:room], got["desc"][:packed], got["index"][:packed], 32)
        assert [b[0].tolist() for b in tx[0]] == [b[0].tolist() for b in want_tx[0]], what
        assert [b[1] for b in tx[0]] == [b[1] for b in want_tx[0]], what
        assert tx[1:] == want_tx[1:]


def test_round_trip(gpu_worker_factory):
    """The packed output is a batch: config_b_small's, with UPE_FRAME_TAIL bytes of room behind
    it, classified where it lies by a second context with the same tables."""
    wl, ref = golden_io.load("config_b_small")
    out, out_desc, _, info = egress.pack_host(ref["frames"], wl.desc, ref["verdict"])
    k, used = int(info["packed"]), int(info["bytes"])
    assert k > 0
    again = dataclasses.replace(wl, frames=np.concatenate([out, np.zeros(FRAME_TAIL, np.uint8)]),
                                desc=out_desc)
    expect = oracle.run_restated(again)
    w, w2 = gpu_worker_factory(wl.capacity), gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        w2.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.run()
        o = Out(w, wl.n, used + FRAME_TAIL)
        w.h2d(o.out, np.zeros(used + FRAME_TAIL, np.uint8))   # the tail is the caller's to size
        w.egress_pack(b.frames, b.desc, b.verdict, wl.n, o.out, used + FRAME_TAIL, o.desc, o.info)
        w.sync()
        verdict2 = w2.malloc(4 * k)
        w2.process(o.out, o.desc, verdict2, k)
        v2 = np.zeros(k, np.uint32)
        w2.sync()
        w2.d2h(v2, verdict2)
        w2.sync()
        got = o.fetch()
        w2.free(verdict2)
        o.free()
        b.free()
    finally:
        w2.close()
        w.close()
    assert int(got["info"]["packed"][0]) == k
    assert np.array_equal(got["desc"][:k], out_desc)
    bad = np.nonzero(v2 != expect.verdict)[0]
    assert bad.size == 0, f"{bad.size} verdicts of the second pass differ, first {bad[:8].tolist()}"
    assert np.array_equal(got["out"][:used + FRAME_TAIL], expect.frames), \
        "the second pass's rewritten frames differ"


def test_empty_batch(gpu_worker_factory):
    """n == 0 zeroes *d_info and launches nothing."""
    w = gpu_worker_factory()
    try:
        before = w.launch_info()["launches"]
        o = Out(w, 0, 64)
        w.egress_pack(0, 0, 0, 0, o.out, 64, o.desc, o.info)
        got = o.fetch()
        o.free()
        assert w.launch_info()["launches"] == before
    finally:
        w.close()
    assert got["info"].tobytes() == bytes(32)
    assert np.all(got["out"] == POISON)


@pytest.mark.parametrize("how", ["null_info", "null_out_desc", "misaligned_out",
                                 "out_inside_frames"])
def test_bad_arguments(gpu_worker_factory, how):
    """-1 with a message and no launch (every output keeps its poison); a valid call after it
    still passes."""
    n = 65
    frames, desc, rec, _, _ = _synthetic(n)
    v = _verdict(n, _patterns(n)["p50"])
    want = egress.pack_host(frames, desc, v)
    room = int(want[3]["need"])
    w = gpu_worker_factory()
    try:
        d = Dev(w, frames, desc, rec)
        d.set_verdict(v)
        o = Out(w, n, room)
        args = {"out": o.out, "out_desc": o.desc, "info": o.info}
        if how == "null_info":
            args["info"] = 0
        elif how == "null_out_desc":
            args["out_desc"] = 0
        elif how == "misaligned_out":
            args["out"] = o.out + 8
        else:
            args["out"] = d.frames + 256
        with pytest.raises(gpu.UpeGpuError) as e:
            w.egress_pack(d.frames, d.desc, d.verdict, n, args["out"], room, args["out_desc"],
                          args["info"], out_index=o.index)
        assert str(e.value).split(":", 1)[1].strip()
        left = o.fetch()
        for k in ("out", "desc", "index", "info"):
            assert np.all(left[k].view(np.uint8) == POISON), f"{k} was written"
        h_frames = np.zeros(frames.nbytes, np.uint8)
        w.d2h(h_frames, d.frames)
        w.sync()
        assert np.array_equal(h_frames, frames), "the frames were written"
        o.free()
        _check(_pack(w, d, n, False, room), want, room, f"after {how}")
        d.free()
    finally:
        w.close()


def test_back_to_back(gpu_worker_factory):
    """Packs of different n queued on one context without a wait between them: the scratch is
    reused (and grown) from one to the next."""
    sizes = [65, 3 * B + 17, B + 1]
    w = gpu_worker_factory()
    devs, outs, wants = [], [], []
    try:
        for n in sizes:
            frames, desc, rec, _, _ = _synthetic(n)
            v = _verdict(n, _patterns(n)["p50"])
            d = Dev(w, frames, desc, rec)
            d.set_verdict(v)
            devs.append(d)
            wants.append(egress.pack_host(frames, desc, v, hdr=rec))
            outs.append(Out(w, n, int(wants[-1][3]["need"])))
        for n, d, o in zip(sizes, devs, outs):
            w.egress_pack(d.frames, d.desc, d.verdict, n, o.out, o.out_bytes, o.desc, o.info,
                          hdr=d.rec, out_index=o.index)
        for n, o, want in zip(sizes, outs, wants):
            _check(o.fetch(), want, o.out_bytes, f"pack of {n} in a queue of three")
        for x in devs + outs:
            x.free()
    finally:
        w.close()

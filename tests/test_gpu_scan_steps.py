"""GPU: the scan kernels of the ordered-output stages past their first step.  Each `*_scan` kernel
is one workgroup that covers 1024 tiles per step and carries a running sum from step to step; the
other GPU tests stay below 1024 tiles, so this file runs every stage at the smallest size whose
scan takes two steps — 1025 tiles, the last a tile of one item — and beside it at exactly 1024
tiles.  Items of interest (control records, replies, forwards, misses, bad handles) lie in tile 0,
in tile 1023 (the last of step one) and in tile 1024 (step two's only tile), and sparsely between,
so that the carry shows in tile 1024's exclusive prefix, in the totals of the info and in the
position of the last output record; for the two stages with a capacity, one case puts the cut into
tile 1024, so that the cut search runs behind a carry.  Expected values are the host twins'
(gpu.ctrl_writes_host, gpu.neigh_patch_host, gpu.release_order_host, egress.pack_host,
ingress.gather_host); every output byte and every info word is compared, nothing else allowed."""
from __future__ import annotations

import numpy as np
import pytest

import ctrl_cases as cc
import neigh_cases as nc
import patch_cases as pc
import release_cases as rc
import resolve_cases as rsc
import test_gpu_egress_pack as eg
import test_gpu_ingress_gather as ig
from test_ctrl_writes import raw
from test_gpu_ctrl_writes import device_call as ctrl_call
from test_gpu_keys import POISON, dev_in
from test_gpu_neigh_patch import A, _info, gpu_patch
from test_gpu_release_order import P32, ROOM, device_call as release_call
from test_gpu_resolve import gpu_resolve
from upe_amd import egress, gpu, ingress
from upe_amd.layout import CW_ARP, CW_NDP, FRAME_TAIL, V_FWD, VF_ARP_REPLY, make_desc

pytestmark = pytest.mark.gpu

STEP = 1024            # tiles per step of every scan kernel (kScanThreads)
TILES = (STEP, STEP + 1)


def items_of(tiles: int, block: int) -> int:
    """The smallest batch of `tiles` tiles when that is one past a step (a last tile of one item),
    else whole tiles."""
    n = block * STEP + 1 if tiles == STEP + 1 else block * tiles
    assert (n + block - 1) // block == tiles
    return n


def marks_of(n: int, block: int, every: int) -> np.ndarray:
    """The positions of interest: the first two items and the last of tile 0, the first and last of
    tile 1023, the batch's last item (tile 1024's only one, when there is a tile 1024), and every
    `every`-th item between."""
    p = {0, 1, block - 1, (STEP - 1) * block, STEP * block - 1, n - 1} | set(range(every, n, every))
    m = np.array(sorted(p))
    assert m[-1] == n - 1 and all(np.any(m // block == t) for t in (0, STEP - 1, (n - 1) // block))
    return m


# ---- upe_gpu_ctrl_writes ---------------------------------------------------------------------

@pytest.mark.parametrize("tiles", TILES)
def test_ctrl_writes(gpu_worker_factory, tiles):
    n = items_of(tiles, gpu.CTRL_BLOCK)
    marks = marks_of(n, gpu.CTRL_BLOCK, 4099)
    kinds = [cc._PLAIN] + [cc._writer(j) for j in range(6)]   # ARP, NS and NA writers
    frames, d = cc.pack([(f, len(f)) for f in kinds])
    which = np.zeros(n, np.int64)
    which[marks] = 1 + np.arange(len(marks)) % 6
    desc = d[which]
    want, winfo = gpu.ctrl_writes_host(frames, desc)
    assert np.array_equal(want["index"], marks) and int(winfo["ctrl"]) == len(marks)
    with gpu_worker_factory(16) as w:
        df, dd = dev_in(w, frames), dev_in(w, desc)
        # everything stored; the last record (tile 1024's, behind the carry) cut off; no room
        for cap in (len(want) + 3, len(want) - 1, 0):
            exp, einfo = gpu.ctrl_writes_host(frames, desc, cap)
            got, ginfo = ctrl_call(w, df, dd, n, cap)
            stored = min(cap, len(want))
            assert int(einfo["stored"]) == stored and int(einfo["writes"]) == len(want)
            assert ginfo.tobytes() == raw(einfo), (cap, ginfo.view(np.uint64), einfo)
            assert got[:32 * stored].tobytes() == raw(exp), cap
            assert (got[32 * stored:] == POISON).all(), f"cap {cap}: a slot past `stored` written"
        w.free(df)
        w.free(dd)


# ---- upe_gpu_release_order -------------------------------------------------------------------

@pytest.mark.parametrize("tiles", TILES)
def test_release_order(gpu_worker_factory, tiles):
    n = items_of(tiles, gpu.RELEASE_BLOCK)
    marks = marks_of(n, gpu.RELEASE_BLOCK, 4099)
    v = rc.words(rc.fwd_mask(n, 3))
    v[marks] |= np.uint32(VF_ARP_REPLY)
    slot = rc.slots(n, "repeat")
    with gpu_worker_factory(16) as w:
        for form in ({"burst": 48}, {"first": rc.SHAPES["straddle_before"](n)}):
            exp = gpu.release_order_host(v, slot=slot, **form)
            info = exp[4]
            assert int(info["replies"]) == len(marks) and int(info["bad_bursts"]) == 0
            assert exp[3][len(marks) - 1] == n - 1   # the last reply: tile 1024's prefix + 0
            got = release_call(w, v, slot=slot, **form)
            assert got[4].tobytes() == info.tobytes(), (form.keys(), got[4].view(np.uint64), info)
            bursts = len(exp[2]) - ROOM
            for name, g, e, k in (("order", got[0], exp[0], n), ("handle", got[1], exp[1], n),
                                  ("burst_fwd", got[2], exp[2], bursts),
                                  ("reply", got[3], exp[3], len(marks))):
                assert len(g) == len(e), name
                assert (e[k:] == gpu.RELEASE_POISON).all(), name
                assert np.array_equal(g[:k], e[:k]), f"{name}: first difference at " \
                    f"{int(np.nonzero(g[:k] != e[:k])[0][0])}"
                assert (g[k:] == P32).all(), f"{name} written from entry {k} on"


# ---- upe_gpu_neigh_patch ---------------------------------------------------------------------

@pytest.mark.parametrize("tiles", TILES)
def test_neigh_patch(gpu_worker_factory, tiles):
    count = items_of(tiles, gpu.PATCH_BLOCK)
    marks = marks_of(count, gpu.PATCH_BLOCK, 1009)
    cs = nc.case(A)
    a4 = [k for k in cs.own("arp") if nc.Probe(cs.arp).slot(k) >= 0][:2]
    a6 = [k for k in cs.own("ndp") if nc.Probe(cs.ndp).slot(k) >= 0][:1]
    base = pc.make([(CW_ARP, a4[0]), (CW_NDP, a6[0]), (CW_ARP, a4[1]),            # held
                    (CW_ARP, 0xDEAD0001), (CW_NDP, bytes(range(0x40, 0x50)))])    # not held
    which = np.arange(count) % 3
    which[marks] = 3 + np.arange(len(marks)) % 2
    recs = base[which].copy()
    r = np.arange(count, dtype=np.uint32)
    recs["index"] = 3 * r + 1
    recs["mac"] = np.stack([np.full(count, 0x0A), np.full(count, 0x5B), r >> 16, r >> 8, r,
                            np.full(count, 0x5C)], axis=1).astype(np.uint8)   # pc.rank_mac
    keys = pc.record_keys(base)
    image = gpu.NeighImage(cs.arp, cs.ndp)
    miss_h, info_h = gpu.neigh_patch_host(image, recs)
    want = gpu.neigh_image_lookup_host(image, rsc.as_keys(keys))
    image.free()
    assert _info(info_h) == (count, count - len(marks), len(marks), 0)
    assert np.array_equal(miss_h, marks)   # the last: workgroup 1024's prefix + 0
    with gpu_worker_factory(16) as w:
        w.load_neigh(cs.arp, cs.ndp)
        miss, info = gpu_patch(w, recs)
        got = gpu_resolve(w, keys)
    assert _info(info) == _info(info_h)
    assert np.array_equal(miss, miss_h)
    assert np.array_equal(got, want), "the patched snapshot answers differently"


# ---- upe_gpu_egress_pack ---------------------------------------------------------------------

def _egress_batch(n, marks):
    """n packets over eight frames (the descriptors repeat), the marked ones forwarded; a record
    per slot."""
    rng = np.random.default_rng(n)
    lens = np.array([60, 64, 65, 128, 1514, 81, 42, 2048])
    padded = (lens + 15) & ~15
    frames = rng.integers(0, 256, int(padded.sum()) + FRAME_TAIL, dtype=np.uint8)
    desc = make_desc(np.cumsum(padded) - padded, lens)[np.arange(n) % len(lens)]
    rec = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    rec[:, 15] = rng.choice([4, 6], n)
    v = rng.choice([0, 1, 2, 3, 5, 6], n).astype(np.uint32)
    v[marks] = V_FWD
    v |= rng.integers(0, 1 << 28, n, dtype=np.uint32) << np.uint32(4)   # flag and rule bits
    return frames, desc, rec, v


@pytest.mark.parametrize("tiles", TILES)
def test_egress_pack(gpu_worker_factory, tiles):
    n = items_of(tiles, gpu.EGRESS_BLOCK)
    marks = marks_of(n, gpu.EGRESS_BLOCK, 4099)
    frames, desc, rec, v = _egress_batch(n, marks)
    w = gpu_worker_factory()
    try:
        d = eg.Dev(w, frames, desc, rec)
        d.set_verdict(v)
        for hdr in (False, True):
            want = egress.pack_host(frames, desc, v, hdr=rec if hdr else None)
            assert np.array_equal(want[2], marks)   # the last entry: tile 1024's prefix + 0
            need = int(want[3]["need"])
            caps = {"room": need + 32}
            if tiles > STEP:
                caps["cut in tile 1024"] = need - 1   # its one packet is the one that does not fit
            for name, cap in caps.items():
                if cap != need + 32:
                    want = egress.pack_host(frames, desc, v, hdr=rec if hdr else None,
                                            out_bytes=cap)
                    assert int(want[3]["packed"]) == len(marks) - 1
                got = eg._pack(w, d, n, hdr, cap)
                eg._check(got, want, cap, f"{tiles} tiles, {name}, {'hdr' if hdr else 'in place'}")
        d.free()
    finally:
        w.close()


# ---- upe_gpu_ingress_gather ------------------------------------------------------------------

def _ingress_burst(n, marks):
    """A pool of six buffers — an empty frame, an ARP request, a neighbour solicitation, three
    plain frames — and n handles: the empty frame's but for the marked ones, which cycle through
    the others and a handle past the pool (a bad one); the last handle is the ARP request's."""
    stride = 2064
    ctl = ig._control_frames()
    rng = np.random.default_rng(n)
    data = [np.zeros(0, np.uint8), ctl[0][0], ctl[3][0]] + \
        [rng.integers(0, 256, k, dtype=np.uint8) for k in (60, 1514, 17)]
    lens = [0, 64, 78, 60, 1514, 17]
    pool = ingress.make_pool(data, lens, range(6), 6, stride, fill=0x3C)
    slots = np.zeros(n, np.uint32)
    slots[marks] = 1 + np.arange(len(marks)) % 6   # 6: outside the pool
    slots[n - 1] = 1
    return pool, stride, slots


@pytest.mark.parametrize("tiles", TILES)
def test_ingress_gather_full(gpu_worker_factory, tiles):
    n = items_of(tiles, gpu.INGRESS_BLOCK)
    marks = marks_of(n, gpu.INGRESS_BLOCK, 4099)
    pool, stride, slots = _ingress_burst(n, marks)
    w = gpu_worker_factory()
    try:
        d_pool = ig._upload(w, pool)
        got, want = ig._run(w, d_pool, pool, stride, slots, ingress.FULL)
        info = want[4]
        assert int(info["packed"]) == n and int(info["bad"]) > 0 and int(info["first_bad"]) > 0
        assert int(info["n_ctrl"]) > 2 and want[3][-1] == n - 1   # tile 1024's prefix + 0
        ig._check(got, want, n, f"{tiles} tiles")
        ig._pool_unchanged(w, d_pool, pool)
        w.free(d_pool)
    finally:
        w.close()


def test_ingress_gather_cut_in_tile_1024(gpu_worker_factory):
    """The capacity one quad short: the batch's last frame, tile 1024's only one, is the one that
    does not fit, so the cut search runs in the scan's second step."""
    n = items_of(STEP + 1, gpu.INGRESS_BLOCK)
    marks = marks_of(n, gpu.INGRESS_BLOCK, 4099)
    pool, stride, slots = _ingress_burst(n, marks)
    rest = ingress.gather_host(pool, stride, slots[marks], ingress.FULL)
    need = int(rest[4]["need"])   # the other handles' frames are empty
    w = gpu_worker_factory()
    try:
        d_pool = ig._upload(w, pool)
        got, want = ig._run(w, d_pool, pool, stride, slots, ingress.FULL, out_bytes=need - 16)
        info = want[4]
        assert int(info["need"]) == need and int(info["packed"]) == n - 1
        assert int(info["bytes"]) == need - 64 and len(want[3]) == int(info["n_ctrl"]) - 1
        ig._check(got, want, n, "cut in tile 1024")
        w.free(d_pool)
    finally:
        w.close()

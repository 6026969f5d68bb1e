"""The control-write calls on the host: upe_amd/ctrl.py (numpy) against the reference worker's own
tables after the golden batches and after the stream the segmented GPU test uses, against the
hand-written expectations of tests/ctrl_cases.py, and against upe_gpu_ingress_gather's marks;
upe_ctrl_writes_host and upe_neigh_apply_writes (upe_host.c) byte for byte against that twin.
No GPU."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import ctrl_cases as cc
import golden_io
import oracle
from upe_amd import ctrl, gpu, ingress, synth
from upe_amd.layout import (ARP_DTYPE, CTRL_INFO_DTYPE, CTRL_WRITE_DTYPE, CW_ARP, CW_NDP,
                            NDP_DTYPE, desc_lens, desc_offsets)

KEEP = ["ip", "mac", "valid"]
NOW = 1234
GOLDENS = ("edge_zero", "edge_consistent", "edge_inconsistent", "ndp_walk", "config_c_small")


def raw(a) -> bytes:
    """The records' bytes with the padding zero (numpy leaves a structured array's padding alone
    in a copy)."""
    a = np.asarray(a)
    if not a.dtype.names:
        return np.ascontiguousarray(a).tobytes()
    out = np.zeros(a.shape, a.dtype)
    for f in a.dtype.names:
        out[f] = a[f]
    return out.tobytes()


def batches():
    """Every ctrl_cases batch: (name, frames, desc)."""
    yield ("chosen",) + cc.chosen_batch()
    yield ("chosen, poisoned",) + cc.chosen_batch(poison=True)
    for n in cc.SIZES:
        for p in cc.PATTERNS:
            yield (f"{p} n={n}",) + cc.placement(n, p)[:2]


# ---- the twin against the reference --------------------------------------------------------

@pytest.mark.parametrize("case", GOLDENS)
def test_goldens_reference_tables(case):
    """The golden's arp / ndp are the reference worker's tables after the batch."""
    wl, ref = golden_io.load(case)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    writes, info = ctrl.ctrl_writes(wl.frames, wl.desc)
    applied = ctrl.apply_writes(arp, ndp, writes, NOW)
    assert np.array_equal(arp[KEEP], ref["arp"][KEEP])
    assert np.array_equal(ndp[KEEP], ref["ndp"][KEEP])
    assert applied == info["writes"] == len(writes)
    if case != "config_c_small":
        assert len(writes) > 0
    for t, t0 in ((arp, wl.arp), (ndp, wl.ndp)):
        changed = (t["valid"] != t0["valid"]) | (t["mac"] != t0["mac"]).any(axis=1)
        assert np.all(t["update_at"][changed] == NOW)
        assert np.all((t["update_at"] == t0["update_at"]) | (t["update_at"] == NOW))


def test_stream_of_the_segmented_test():
    wl = cc.with_control(synth.config_c(n=4000, seed=31), 40, 31)
    r = oracle.run_reference(wl) if oracle.ref_available() else \
        oracle.run_restated(wl, apply_control=True)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    writes, info = ctrl.ctrl_writes(wl.frames, wl.desc)
    ctrl.apply_writes(arp, ndp, writes, NOW)
    assert 0 < info["writes"] < info["ctrl"] < 40   # ARP with hlen 8: no mark; NS bare: no record
    assert np.array_equal(arp[KEEP], r.arp[KEEP])
    assert np.array_equal(ndp[KEEP], r.ndp[KEEP])


def test_chosen_frames_by_hand():
    items = cc.chosen()
    for poison in (False, True):
        frames, desc = cc.chosen_batch(poison)
        writes, info = ctrl.ctrl_writes(frames, desc)
        by_index = {int(w["index"]): w for w in writes}
        marked = ctrl.marks(frames, desc)
        for i, (label, _, _, want) in enumerate(items):
            assert bool(marked[i]) == (want != cc.NOT_MARKED), label
            if isinstance(want, str):
                assert i not in by_index, label
                continue
            w = by_index[i]
            got = (int(w["kind"]), int(w["mac_off"]), bytes(w["mac"]), bytes(w["ip"]))
            assert got == want, label
            assert w["zero0"] == 0 and w["zero1"] == 0
        assert info["ctrl"] == sum(want != cc.NOT_MARKED for *_, want in items)
        assert info["writes"] == len(writes) == sum(not isinstance(want, str) for *_, want in items)
        assert list(writes["index"]) == sorted(by_index)
    kinds = {want[0] for *_, want in items if not isinstance(want, str)}
    assert kinds == {CW_ARP, CW_NDP}


def test_poison_changes_nothing():
    a, b = cc.chosen_batch(), cc.chosen_batch(poison=True)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    wa, ia = ctrl.ctrl_writes(*a)
    wb, ib = ctrl.ctrl_writes(*b)
    assert raw(wa) == raw(wb) and raw(ia) == raw(ib) and len(wa) > 20


@pytest.mark.parametrize("n", cc.SIZES)
def test_placement_twin(n):
    for p in cc.PATTERNS:
        frames, desc, pos = cc.placement(n, p)
        writes, info = ctrl.ctrl_writes(frames, desc)
        assert np.array_equal(writes["index"], pos), p
        assert info["ctrl"] == info["writes"] == info["stored"] == len(pos)
        assert info["first_write"] == (pos[0] if len(pos) else ctrl.NONE)
        # each writer names its position in its MAC
        assert all(int.from_bytes(bytes(w["mac"][2:]), "big") == w["index"] for w in writes)


# ---- the C twins -----------------------------------------------------------------------------

def _tables(seed, full=False):
    """Small tables (collisions, wrap-around), part filled; full: every slot valid."""
    rng = np.random.default_rng(seed)
    arp, ndp = np.zeros(8, ARP_DTYPE), np.zeros(4, NDP_DTYPE)
    for t in (arp, ndp):
        k = len(t) if full else len(t) // 2
        s = rng.permutation(len(t))[:k]
        t["valid"][s] = 1
        t["ip"][s] = rng.integers(0, 256, t["ip"][s].shape).astype(t["ip"].dtype)
        t["mac"][s] = rng.integers(0, 256, (k, 6))
        t["update_at"][s] = 7
    return arp, ndp


def test_host_twins_every_batch():
    for name, frames, desc in batches():
        want, winfo = ctrl.ctrl_writes(frames, desc)
        got, ginfo = gpu.ctrl_writes_host(frames, desc)
        assert raw(got) == raw(want), name
        assert raw(ginfo) == raw(winfo), name
        for k, (full, big) in enumerate(((False, False), (True, False), (False, True))):
            a0, n0 = _tables(k, full)
            if big:
                a0, n0 = np.zeros(4096, ARP_DTYPE), np.zeros(4096, NDP_DTYPE)
            a1, n1 = a0.copy(), n0.copy()
            assert gpu.neigh_apply_writes(a0, n0, got, NOW) == ctrl.apply_writes(a1, n1, want, NOW)
            assert raw(a0) == raw(a1) and raw(n0) == raw(n1), name
        # one family without a table: its records are not counted
        a0, _ = _tables(3)
        a1 = a0.copy()
        applied = gpu.neigh_apply_writes(a0, None, got, NOW)
        assert applied == ctrl.apply_writes(a1, None, want, NOW) == int((want["kind"] == CW_ARP).sum())
        assert raw(a0) == raw(a1)


def test_update_at_exactly_on_the_slots_written():
    frames, desc = cc.chosen_batch()
    writes, _ = gpu.ctrl_writes_host(frames, desc)
    a0, n0 = np.zeros(64, ARP_DTYPE), np.zeros(64, NDP_DTYPE)
    a0["update_at"], n0["update_at"] = 7, 7
    a, n = a0.copy(), n0.copy()
    assert gpu.neigh_apply_writes(a, n, writes, NOW) == len(writes)
    for t, t0 in ((a, a0), (n, n0)):
        written = t["valid"] != 0
        assert written.any() and np.all(t["update_at"][written] == NOW)
        assert raw(t[~written]) == raw(t0[~written])
    # a full table of other addresses is left alone, and still counted
    fa, fn = _tables(5, full=True)   # addresses 0..255 / random bytes: none of the records'
    assert not np.isin(writes["ip"][:, :4].copy().view("<u4").ravel(), fa["ip"]).any()
    ka, kn = fa.copy(), fn.copy()
    assert gpu.neigh_apply_writes(fa, fn, writes, NOW) == len(writes)
    assert raw(fa) == raw(ka) and raw(fn) == raw(kn)
    assert ctrl.apply_writes(ka, kn, writes, NOW) == len(writes)
    assert raw(fa) == raw(ka) and raw(fn) == raw(kn)


def test_info_ctrl_equals_the_ingress_marks():
    for name, frames, desc in batches():
        offs, lens = desc_offsets(desc), desc_lens(desc)
        first = frames[np.minimum(offs[:, None] + np.arange(55), frames.size - 1)]
        m = ingress.table_writes(first, lens)
        _, info = ctrl.ctrl_writes(frames, desc)
        assert info["ctrl"] == np.count_nonzero(m), name
        assert np.array_equal(ctrl.marks(frames, desc), m), name
    # and through a pool, as upe_gpu_ingress_gather sees the same frames
    items = [(f, ln) for _, f, ln, _ in cc.chosen()]
    frames, desc = cc.pack(items)
    stride = 2064
    pool = ingress.make_pool([np.frombuffer(f, np.uint8) for f, _ in items],
                             [ln for _, ln in items], range(len(items)), len(items), stride,
                             fill=0xFF)
    _, _, _, positions, ginfo = ingress.gather_host(pool, stride, np.arange(len(items)), ingress.REF)
    _, info = ctrl.ctrl_writes(frames, desc)
    assert info["ctrl"] == ginfo["n_ctrl"]
    assert np.array_equal(positions, np.nonzero(ctrl.marks(frames, desc))[0])


# ---- layout and refusals -------------------------------------------------------------------

def test_layout():
    assert CTRL_WRITE_DTYPE.itemsize == 32 and CTRL_INFO_DTYPE.itemsize == 32
    f = CTRL_WRITE_DTYPE.fields
    assert [f[k][1] for k in ("index", "kind", "zero0", "mac_off", "mac", "zero1", "ip")] == \
        [0, 4, 5, 6, 8, 14, 16]
    assert (CW_ARP, CW_NDP) == (4, 6) and gpu.CTRL_BLOCK == cc.BLOCK == ctrl.CTRL_BLOCK == 1024
    assert gpu.CTRL_WRITE_DTYPE is CTRL_WRITE_DTYPE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "upe_gpu.h")).read()
    for line in ("#define UPE_CTRL_BLOCK 1024", "enum { UPE_CW_ARP = 4, UPE_CW_NDP = 6 };",
                 "sizeof(upe_ctrl_write_t) == 32", "offsetof(upe_ctrl_write_t, mac_off) == 6",
                 "offsetof(upe_ctrl_write_t, mac) == 8", "offsetof(upe_ctrl_write_t, ip) == 16",
                 "sizeof(upe_ctrl_info_t) == 32"):
        assert line in src, line


def test_cap_truncation_is_a_prefix():
    frames, desc = cc.chosen_batch()
    full, finfo = gpu.ctrl_writes_host(frames, desc)
    total = len(full)
    for cap in (0, 1, total - 1, total, total + 7):
        for fn in (gpu.ctrl_writes_host, ctrl.ctrl_writes):
            got, info = fn(frames, desc, cap)
            assert raw(got) == raw(full[:cap])
            assert info["stored"] == min(cap, total) and info["writes"] == total
            assert info["ctrl"] == finfo["ctrl"] and info["first_write"] == finfo["first_write"]
    # nothing at or past writes + cap is written
    L = gpu.LIB
    buf = np.full(total + 4, 0xA7, np.uint8).repeat(32).view(CTRL_WRITE_DTYPE)
    info = np.zeros(1, CTRL_INFO_DTYPE)
    assert L.upe_ctrl_writes_host(frames.ctypes.data, desc.ctypes.data, len(desc),
                                  buf.ctypes.data, total - 1, info.ctypes.data) == 0
    assert raw(buf[:total - 1]) == raw(full[:total - 1])
    assert set(raw(buf[total - 1:])) == {0xA7}


def test_empty_batch():
    w, info = gpu.ctrl_writes_host(np.zeros(96, np.uint8), np.zeros(0, np.uint64))
    w2, info2 = ctrl.ctrl_writes(np.zeros(96, np.uint8), np.zeros(0, np.uint64))
    assert len(w) == len(w2) == 0 and raw(info) == raw(info2)
    assert info["first_write"] == ctrl.NONE and info["ctrl"] == info["writes"] == info["stored"] == 0


def test_refused_arguments_change_nothing():
    L = gpu.LIB
    frames, desc = cc.chosen_batch()
    writes, _ = gpu.ctrl_writes_host(frames, desc)
    F, D, n = frames.ctypes.data, desc.ctypes.data, len(desc)
    out = np.full(32 * 8, 0xA7, np.uint8)
    info = np.full(32, 0xA7, np.uint8)
    O, I = out.ctypes.data, info.ctypes.data
    for args in ((None, D, n, O, 8, I), (F, None, n, O, 8, I), (F, D, n, O, 8, None),
                 (F, D, n, None, 8, I), (F, D, (1 << 32) - 1024, O, 8, I)):
        assert L.upe_ctrl_writes_host(*args) == -1
        assert b"upe_ctrl_writes_host" in L.upe_host_last_error()
    assert set(out) == {0xA7} and set(info) == {0xA7}
    # apply: everything is checked before the first write
    arp, ndp = _tables(9)
    a0, n0 = arp.copy(), ndp.copy()
    bad = writes.copy()
    bad["kind"][-1] = 5
    applied = ctypes.c_size_t(77)
    A, N, W = arp.ctypes.data, ndp.ctypes.data, writes.ctypes.data
    for args in ((A, 8, N, 4, bad.ctypes.data, len(bad)),   # an unknown kind, last
                 (A, 6, N, 4, W, len(writes)),              # a capacity that is no power of two
                 (A, 8, N, 3, W, len(writes)),
                 (None, 8, N, 4, W, len(writes)),           # a missing table
                 (A, 8, None, 4, W, len(writes)),
                 (A, 8, N, 4, None, len(writes))):
        assert L.upe_neigh_apply_writes(*args, NOW, ctypes.byref(applied)) == -1
        assert b"upe_neigh_apply_writes" in L.upe_host_last_error()
    assert raw(arp) == raw(a0) and raw(ndp) == raw(n0) and applied.value == 77
    with pytest.raises(ValueError):
        ctrl.apply_writes(arp, ndp, bad, NOW)
    with pytest.raises(ValueError):
        ctrl.apply_writes(arp[:6], ndp, writes, NOW)
    assert raw(arp) == raw(a0) and raw(ndp) == raw(n0)
    # no table at all: nothing to apply to, nothing counted
    assert L.upe_neigh_apply_writes(None, 0, None, 0, W, len(writes), NOW,
                                    ctypes.byref(applied)) == 0 and applied.value == 0

"""The gate matrix (tests/gates.py) on the CPU: its expected values deserve trust, and it is not
hollow, before any GPU is involved.

The C restatement (oracle/cpu_ref.c) copies a frame's first `len` bytes into a zeroed buffer, so
it cannot see what lies past `len`: its answers must be the same under all four fills, and the
fill must still stand behind every frame afterwards.  Where the reference worker itself is built
(oracle/_ref), it agrees on every fill.  The matrix reaches every verdict code and flag, most
truncated frames would get another answer if their tail were read, and every IHL x L4 kind has
the three lengths around its last gate."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import gates
import oracle
from upe_amd import rx
from upe_amd.layout import (VF_ARP_LEARN, VF_ARP_REPLY, VF_L1_INIT, VF_NEIGH_HIT, desc_lens,
                            desc_offsets)


@functools.lru_cache(maxsize=None)
def _matrix(fill, order="grouped"):
    return gates.matrix(fill, order)


@functools.lru_cache(maxsize=None)
def _restated(fill, order, apply_control):
    return oracle.run_restated(_matrix(fill, order)[0], apply_control=apply_control)


def _tail_mask(wl):
    """True for every byte of the frames buffer that is at or past its frame's len."""
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    m = np.ones(wl.frames.shape[0], bool)
    for o, ln in zip(offs, lens):
        m[o:o + ln] = False
    return m


def _fill_bytes(sid, fill):
    """The buffer as gates.pack filled it before any frame was written."""
    return gates.pack([(b"", 0, gates.SHAPES[i].data) for i in sid], fill)[0]


def _same(a, b, what):
    assert np.array_equal(a.verdict, b.verdict), f"{what}: verdicts"
    assert a.counters.tobytes() == b.counters.tobytes(), f"{what}: counters"
    assert np.array_equal(a.rule_stats, b.rule_stats), f"{what}: rule_stats"
    assert a.l1.tobytes() == b.l1.tobytes(), f"{what}: L1"


def test_matrix_size():
    wl, parent, sid, trunc = _matrix("zero")
    assert wl.n < gates.MAX_FRAMES and wl.frames.nbytes < 4 << 20
    assert len(wl.rules) >= 61
    assert parent.shape == sid.shape == trunc.shape == (wl.n,)
    lens = desc_lens(wl.desc)
    for i, s in enumerate(gates.SHAPES):
        mine = np.sort(lens[sid == i])
        want = np.arange(len(s.data) + 1) if s.multi else np.array([len(s.data)])
        assert np.array_equal(mine, want), s.name     # every truncation, not samples
    for order in gates.ORDERS:   # the generator is deterministic
        a, b = gates.matrix("random", order)[0], _matrix("random", order)[0]
        assert np.array_equal(a.frames, b.frames) and np.array_equal(a.desc, b.desc)
    sub = gates.boundary_subset("parent")[0]
    ctl = gates.control_subset("parent")[0]
    assert 0 < sub.n <= gates.MAX_SUBSET and 0 < ctl.n <= gates.MAX_SUBSET


@pytest.mark.parametrize("apply_control", [False, True])
@pytest.mark.parametrize("order", gates.ORDERS)
def test_restated_oracle_is_fill_independent(order, apply_control):
    base = _restated("zero", order, apply_control)
    for fill in gates.FILLS:
        wl, _, sid, _ = _matrix(fill, order)
        r = _restated(fill, order, apply_control)
        _same(r, base, f"{fill} {order} apply_control={apply_control}")
        tail = _tail_mask(wl)
        # the frames differ between fills only past len, and there the fill still stands
        assert np.array_equal(r.frames[~tail], base.frames[~tail]), fill
        assert np.array_equal(r.frames[tail], _fill_bytes(sid, fill)[tail]), \
            f"{fill}: a byte at or past len was written"
        if apply_control:
            assert np.array_equal(r.arp, base.arp) and np.array_equal(r.ndp, base.ndp)


def _without_control(wl, verdict):
    """The workload without its table-writing control packets (ARP with the Ethernet / IPv4
    header, NS / NA): what the reference worker, which applies such writes at once, can be
    compared on against the deferred-write restatement."""
    keep = ((verdict & 0xF) != 5) & ((verdict & VF_ARP_LEARN) == 0)
    out = wl.copy()
    out.desc = wl.desc[keep]
    return out


@pytest.mark.parametrize("order", gates.ORDERS)
def test_reference_worker_agrees(order):
    if not oracle.ref_available():
        pytest.skip("the reference worker is not built here")
    first = None
    for fill in gates.FILLS:
        full = _matrix(fill, order)[0]
        wl = _without_control(full, _restated(fill, order, False).verdict)
        assert 0.8 * full.n < wl.n < full.n
        r = oracle.run_restated(wl, apply_control=False)
        ref = oracle.run_reference(wl)
        assert np.array_equal(ref.frames, r.frames), fill
        # (UPE_VF_L1_INIT is this library's flag, not the reference's: test_gpu_fuzz.py)
        assert np.array_equal(ref.verdict & ~np.uint32(0x80), r.verdict & ~np.uint32(0x80)), fill
        assert ref.counters.tobytes() == r.counters.tobytes(), fill
        assert np.array_equal(ref.rule_stats, r.rule_stats), fill
        assert ref.l1.tobytes() == r.l1.tobytes(), fill
        first = first or ref
        assert np.array_equal(ref.verdict, first.verdict), f"{fill}: the reference saw the tail"


def test_reference_worker_agrees_on_control_subset():
    if not oracle.ref_available():
        pytest.skip("the reference worker is not built here")
    keep = ["ip", "mac", "valid"]
    for fill in gates.FILLS:
        wl = gates.control_subset(fill)[0]
        r = oracle.run_restated(wl, apply_control=True)
        ref = oracle.run_reference(wl)
        assert np.array_equal(ref.frames, r.frames), fill
        assert np.array_equal(ref.verdict & ~np.uint32(0x80), r.verdict & ~np.uint32(0x80)), fill
        assert ref.counters.tobytes() == r.counters.tobytes(), fill
        assert np.array_equal(ref.rule_stats, r.rule_stats), fill
        assert np.array_equal(ref.arp[keep], r.arp[keep]), fill
        assert np.array_equal(ref.ndp[keep], r.ndp[keep]), fill


def test_control_subset_learning_matters():
    """The subset is fill-independent in the oracle, writes tables, and the writes change how
    the probes are forwarded."""
    base = None
    for fill in gates.FILLS:
        wl, parent, sid, trunc = gates.control_subset(fill)
        r = oracle.run_restated(wl, apply_control=True)
        base = base or r
        _same(r, base, fill)
        assert np.array_equal(r.arp, base.arp) and np.array_equal(r.ndp, base.ndp)
    frozen = oracle.run_restated(wl, apply_control=False)
    assert not np.array_equal(frozen.frames, r.frames)
    assert not np.array_equal(r.arp, wl.arp) and not np.array_equal(r.ndp, wl.ndp)
    assert set(gates.SHAPES[i].control for i in sid[sid >= 0]) == {"arp", "ns", "na"}


def test_matrix_is_not_hollow():
    wl, parent, sid, trunc = _matrix("parent")
    r = _restated("parent", "grouped", False)
    code = r.verdict & 0xF
    assert set(np.unique(code).tolist()) == set(range(7)), np.bincount(code, minlength=7)
    for flag in (VF_NEIGH_HIT, VF_ARP_LEARN, VF_ARP_REPLY, VF_L1_INIT):
        assert np.any(r.verdict & flag), hex(flag)
    # a truncated frame whose verdict differs from its own bytes' verdict at parent_len: reading
    # past len changes the answer (under the `parent` fill the whole parent is there to be read)
    lens = desc_lens(wl.desc)
    whole = {int(s): int(r.verdict[i]) for i, s in enumerate(sid) if lens[i] == parent[i]
             and gates.SHAPES[int(s)].multi}
    differs = np.array([int(r.verdict[i]) != whole[int(sid[i])] for i in np.nonzero(trunc)[0]])
    assert differs.size > 4000
    assert differs.mean() >= 0.5, differs.mean()
    # both look-back outcomes: a packet to the starting entry's address that takes its MAC, and
    # one that takes the table's
    l1 = wl.l1
    offs = desc_offsets(wl.desc)
    init = np.nonzero((r.verdict & VF_L1_INIT) != 0)[0]
    macs = {bytes(r.frames[offs[i]:offs[i] + 6]) for i in init}
    assert bytes(l1["last_arp_mac"][0]) in macs and bytes(l1["last_ndp_mac"][0]) in macs


def test_gate_triples_present():
    """For each IHL 5..15 and each L4 kind (and each IPv6 kind): min_parse as the oracle's parser
    itself finds it equals the shape's, and the matrix holds min_parse - 1, min_parse and
    min_parse + 1."""
    wl, parent, sid, trunc = _matrix("zero")
    lens = desc_lens(wl.desc)
    seen = set()
    for i in gates.PARSING:
        s = gates.SHAPES[i]
        ok = [oracle.parse(s.data, ln)[0] == 0 for ln in range(len(s.data) + 1)]
        assert ok.index(True) == s.min_parse and all(ok[s.min_parse:]), s.name
        have = set(lens[sid == i].tolist())
        assert {s.min_parse - 1, s.min_parse, s.min_parse + 1} <= have, s.name
        seen.add((s.family, s.ihl, s.l4))
    for ihl in range(5, 16):
        for l4 in ("udp", "tcp5", "tcp15", "icmp", "ff"):
            assert (4, ihl, l4) in seen
    for l4 in ("udp", "tcp5", "tcp8", "icmp"):
        assert (6, 0, l4) in seen


def hashes_of(wl):
    """The reference's parse result and flow hash per frame, as test_gpu_rx_dispatch._draw_d."""
    lib = oracle.oracle_lib()
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    hashes, ok = np.zeros(wl.n, np.uint32), np.zeros(wl.n, bool)
    for i in range(wl.n):
        fr = bytes(wl.frames[offs[i]:offs[i] + min(int(lens[i]), 2048)])
        rc, key = oracle.parse(fr, int(lens[i]))
        if rc == 0:
            ok[i] = True
            hashes[i] = lib.upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p))
    return hashes, ok


@pytest.mark.parametrize("order", gates.ORDERS)
def test_rx_dispatch_is_fill_independent(order):
    base = None
    for fill in gates.FILLS:
        hashes, ok = hashes_of(_matrix(fill, order)[0])
        got = [rx.dispatch_host(hashes, ok, rings, 3) for rings in (4, 64)]
        if base is None:
            base = (hashes, ok, got)
            assert 3 * len(gates.PARSING) <= ok.sum() < ok.size // 2
            assert np.unique(hashes[ok]).size > len(gates.PARSING) // 2
            continue
        assert np.array_equal(hashes, base[0]) and np.array_equal(ok, base[1]), fill
        for a, b in zip(got, base[2]):
            for x, y in zip(a[:3], b[:3]):
                assert np.array_equal(x, y), fill

"""tests/rx_cases.py pinned, without a GPU: the pool's frames against the reference's parse and
hash, every pattern against what it is named for, three dispatches written out by hand, and
rx.dispatch_host against the sequential loop of tests/test_rx_dispatch.py over every pattern, small
size, ring count and starting cursor."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
import rx_cases as rc
from test_rx_dispatch import sequential
from upe_amd import gpu, rx
from upe_amd.layout import FRAME_TAIL, desc_lens, desc_offsets

NV, NP = len(rc.VARIANTS), rc.RING_IDS * len(rc.VARIANTS)


def test_constants():
    assert rc.BLOCK == gpu.RX_BLOCK and rc.RING_IDS == rx.RINGS_MAX == gpu.RX_RINGS_MAX
    assert rc.SCAN_STEP * rc.BLOCK in rc.LARGE and max(rc.SMALL) == 9 * rc.BLOCK
    assert set(rc.LARGE_PATTERNS) | set(rc.CLOSED) <= set(rc.PATTERNS)
    assert [rc.rr_starts(w) for w in (1, 2, 64)] == [[0], [0, 1], [0, 51, 63]]


def test_pool_layout():
    frames, desc = rc.pool()
    offs, lens = desc_offsets(desc), desc_lens(desc)
    assert len(desc) == NP + len(rc.FALLBACKS) and not (offs & 15).any()
    assert np.all(offs[1:] >= offs[:-1] + np.maximum(lens[:-1], 16))   # no two frames overlap
    assert frames.size - int(offs[-1]) - max(int(lens[-1]), 16) >= FRAME_TAIL
    for (_, f, ln), o in zip(rc.pool_items(), offs):
        assert bytes(frames[o:o + len(f)]) == f and ln <= len(f)


def test_pool_frames_against_the_reference():
    items = rc.pool_items()
    hashes, ok = rc.pool_hashes()
    assert ok[:NP].all() and not ok[NP:].any() and not hashes[NP:].any()
    assert np.array_equal(hashes[:NP] & 63, np.arange(NP) // NV), "a frame misses its ring id"
    for r in range(rc.RING_IDS):
        assert len(set(hashes[NV * r:NV * r + NV].tolist())) == NV, f"ring {r}: equal hashes"
    # the bits above the ring id are real values: every mask the dispatch can apply cuts some
    assert len(set((hashes[:NP] >> 6).tolist())) > NP * 3 // 4
    # one by one through the oracle library, by name: family, protocol, and what fails
    lib = oracle.oracle_lib()
    for j, (name, f, ln) in enumerate(items):
        rcode, key = oracle.parse(f, ln)
        assert (rcode == 0) == (j < NP), name
        if j < NP:
            assert int(lib.upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p))) == hashes[j]
            assert (int(key[0]), int(key[40])) == {"udp4": (4, 17), "tcp4": (4, 6),
                                                   "icmp4": (4, 1), "udp6": (6, 17)}[name.split()[0]]
    assert [k for k, _, _ in items[NP:]] == list(rc.FALLBACKS)
    lens = {k: ln for k, _, ln in items[NP:]}
    assert lens["runt"] == 10 and lens["udp4_cut"] == 14 + 20 + 8 - 1
    whole = items[NP + rc.FALLBACKS.index("udp4_cut")][1]
    assert rc.ref_hash(whole)[0], "the cut frame parses when it is whole"
    if oracle.ref_available():   # the compiled reference's parse_flow_key and flow_hash
        fn = oracle.ref_lib().upe_refh_flow_hash
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        frames, desc = rc.pool()
        h, k = np.zeros(len(desc), np.uint32), np.zeros(len(desc), np.uint8)
        assert fn(frames.ctypes.data, desc.ctypes.data, len(desc), h.ctypes.data,
                  k.ctypes.data) == 0
        assert np.array_equal(h, hashes) and np.array_equal(k.astype(bool), ok)


def test_key_layout_used_above():
    """Byte 0 of flow_key_t is ip_ver, byte 40 the protocol."""
    from upe_amd.layout import FLOW_KEY_DTYPE

    assert FLOW_KEY_DTYPE.fields["ip_ver"][1] == 0 and FLOW_KEY_DTYPE.fields["protocol"][1] == 40


@pytest.mark.parametrize("rings", rc.RINGS)
def test_patterns_reach_what_they_are_named_for(rings):
    B = rc.BLOCK
    for n in rc.SMALL + rc.LARGE:
        i = np.arange(n)
        a = {p: rc.assignment(n, rings, p) for p in rc.PATTERNS}
        for p, (kind, ring) in a.items():
            assert kind.shape == ring.shape == (n,), p
            fb = kind == rc.FALLBACK
            assert np.all(ring[fb] == -1) and np.all((ring[~fb] >= 0) & (ring[~fb] < rings)), p
        used = {p: set(ring[kind == rc.PARSED].tolist()) for p, (kind, ring) in a.items()}
        fbs = {p: np.nonzero(kind == rc.FALLBACK)[0] for p, (kind, _) in a.items()}
        assert used["one_ring"] == {rings - 1} and fbs["one_ring"].size == 0   # the others empty
        assert fbs["all_fallback"].size == n
        assert fbs["first_fallback"].tolist() == [0] and fbs["last_fallback"].tolist() == [n - 1]
        assert np.array_equal(fbs["alternate"], i[1::2])
        for p in ("lane_ring", "wave_ring", "tile_ring"):
            assert fbs[p].size == 0
        ring = a["lane_ring"][1]
        assert np.array_equal(ring, i % rings)
        if rings == 64:   # every full wave holds 64 different rings
            full = ring[:n // 64 * 64].reshape(-1, 64)
            assert np.all(np.sort(full, axis=1) == np.arange(64))
        ring = a["wave_ring"][1]
        full = ring[:n // 64 * 64].reshape(-1, 64)
        assert np.all(full == full[:, :1]) and np.array_equal(full[:, 0], np.arange(n // 64) % rings)
        ring = a["tile_ring"][1]   # a tile's whole count in one column
        for t in range(0, min(n, 70 * B), B):
            assert np.all(ring[t:t + B] == (t // B) % rings)
        assert np.array_equal(ring, (i // B) % rings)
        # the fallbacks of edge_fallback are exactly the tile edges
        edges = sorted([b - 1 for b in range(B, n, B)] + list(range(B, n, B)))
        assert fbs["edge_fallback"].tolist() == edges
        kind, ring = a["edge_fallback"]
        assert np.array_equal(ring[kind == rc.PARSED], a["wave_ring"][1][kind == rc.PARSED])
        # runs: both kinds alternate, in runs of the drawn lengths
        kind = a["runs"][0].astype(np.int64)
        cuts = np.nonzero(np.diff(kind))[0] + 1
        lens = np.diff(np.concatenate([[0], cuts]))          # every run but the last, cut by n
        assert set(lens.tolist()) <= set(rc.RUNS)
        if n >= 4097:   # past sum(RUNS): every length, and both kinds
            assert set(lens.tolist()) == set(rc.RUNS) and len(used["runs"]) == rings
            assert 1 + 63 + 64 <= fbs["runs"].size <= n - (1 + 63 + 64)
        if n >= 64 * 64:
            assert used["seeded"] == set(range(rings)), "seeded leaves a ring empty"
            assert 0.05 * n < fbs["seeded"].size < 0.20 * n
            ring = a["seeded"][1]   # half on ring 0, and ring 0's share of the uniform half
            assert abs((ring == 0).sum() / (ring >= 0).sum() - (0.5 + 0.5 / rings)) < 0.05


@pytest.mark.parametrize("rings", rc.RINGS)
def test_batches_follow_their_assignment(rings):
    """A batch's reference values are the pool's, and they say what the assignment chose; over
    the sizes, every ring id, variant and fallback frame is drawn."""
    frames, pdesc = rc.pool()
    hashes, ok = rc.pool_hashes()
    by_desc = {int(d): j for j, d in enumerate(pdesc)}
    seen = set()
    for n in rc.SMALL + rc.LARGE[-1:]:
        for p in rc.PATTERNS if n in rc.SMALL else rc.LARGE_PATTERNS:
            kind, ring = rc.assignment(n, rings, p)
            desc, h, k = rc.batch(n, rings, p)
            assert desc.dtype == np.uint64 and h.dtype == np.uint32 and k.dtype == bool
            assert np.array_equal(k, kind == rc.PARSED), (n, p)
            assert np.array_equal((h & np.uint32(rings - 1))[k], ring[k]), (n, p)
            assert not h[~k].any()
            uniq, first = np.unique(desc, return_index=True)
            fid = np.array([by_desc[int(d)] for d in uniq])
            assert np.array_equal(hashes[fid], h[first]) and np.array_equal(ok[fid], k[first])
            seen.update(fid.tolist())
            d2, h2, k2 = rc.batch(n, rings, p)   # the same batch every time
            assert np.array_equal(desc, d2) and np.array_equal(h, h2) and np.array_equal(k, k2)
    assert seen == set(range(len(pdesc)))


@pytest.mark.parametrize("rings", rc.RINGS)
@pytest.mark.parametrize("pattern", rc.CLOSED)
def test_closed_forms(pattern, rings):
    for n in rc.SMALL + rc.LARGE[3:4]:
        _, h, k = rc.batch(n, rings, pattern)
        for rr in rc.rr_starts(rings) if pattern == "all_fallback" else (rings - 1,):
            ring, index, counts = rc.closed_form(n, rings, pattern, rr)
            got = rx.dispatch_host(h, k, rings, rr)
            assert np.array_equal(got[0], ring), (n, rr)
            assert np.array_equal(got[1], index), (n, rr)
            assert np.array_equal(got[2], counts), (n, rr)
            assert got[3] == (rr + (n if pattern == "all_fallback" else 0)) & (rings - 1)
    # and spelled out once
    ring, index, counts = rc.closed_form(5, 4, "all_fallback", 3)
    assert (ring & 63).tolist() == [3, 0, 1, 2, 3] and index.tolist() == [1, 2, 3, 0, 4]
    assert counts.tolist() == [1, 1, 1, 2, 5]
    ring, index, counts = rc.closed_form(2 * rc.BLOCK + 1, 2, "tile_ring", 0)
    assert index[rc.BLOCK:rc.BLOCK + 2].tolist() == [2 * rc.BLOCK, rc.BLOCK]
    assert counts.tolist() == [rc.BLOCK + 1, rc.BLOCK, 0]


@pytest.mark.parametrize("rings", rc.RINGS)
@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_dispatch_host_equals_the_sequential_loop(pattern, rings):
    for n in rc.SMALL:
        _, h, k = rc.batch(n, rings, pattern)
        for rr_start in (0, rings - 1, 0x7FFFFFF3):
            ring, index, counts, rr_next = rx.dispatch_host(h, k, rings, rr_start)
            want_ring, want_lists, want_rr = sequential(h, k, rings, rr_start & (rings - 1))
            assert np.array_equal(ring, want_ring), (n, rr_start)
            assert rr_next == want_rr
            assert counts.tolist() == [len(x) for x in want_lists] + [int((~k).sum())]
            assert index.tolist() == [i for x in want_lists for i in x], (n, rr_start)

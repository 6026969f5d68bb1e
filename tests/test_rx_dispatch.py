"""rx.dispatch_host, the numpy restatement of the RX thread's dispatch, against a plain sequential
loop that restates pcap_callback's ring choice with its static cursor (reference
src/rx_pcap.c:19-25,67-80), over the reference's own parse results and hashes
(tests/golden/flow_hash.npz).  No GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import golden_io
from upe_amd import rx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("config_a", "config_b_small", "config_c_small", "config_cf_small", "config_d_small",
         "edge_zero", "ndp_walk")
RINGS = (1, 2, 4, 8, 16, 32, 64)
# fallback packets per case (parse_flow_key fails): the round-robin path is exercised
FALLBACKS = {"config_c_small": 354, "config_d_small": 295, "edge_zero": 328, "ndp_walk": 24}


def sequential(hashes, ok, rings, rr):
    """pcap_callback's ring choice, one packet at a time; rr is pick_ring_round_robin's static."""
    ring, lists = [], [[] for _ in range(rings)]
    for i, (h, k) in enumerate(zip(hashes.tolist(), ok.tolist())):
        if k:
            r = h & (rings - 1)
            ring.append(r)
        else:
            r = rr
            rr = (rr + 1) & (rings - 1)
            ring.append(r | rx.FALLBACK)
        lists[r].append(i)
    return np.array(ring, np.uint32), lists, rr


def _params():
    return [(c, w, s) for c in CASES for w in RINGS for s in sorted({0, w - 1})]


def test_fallback_counts_of_the_golden_cases():
    for case, want in FALLBACKS.items():
        _, ok = golden_io.flow_hash(case)
        assert int((~ok.astype(bool)).sum()) == want, case


@pytest.mark.parametrize("case,rings,rr_start", _params())
def test_dispatch_host_equals_the_sequential_loop(case, rings, rr_start):
    hashes, ok = golden_io.flow_hash(case)
    n = len(hashes)
    ring, index, counts, rr_next = rx.dispatch_host(hashes, ok, rings, rr_start)
    want_ring, want_lists, want_rr = sequential(hashes, ok, rings, rr_start)
    assert ring.dtype == np.uint32 and index.dtype == np.uint32 and counts.dtype == np.uint64
    assert np.array_equal(ring, want_ring)
    assert rr_next == want_rr
    assert counts.tolist() == [len(x) for x in want_lists] + [int((~ok.astype(bool)).sum())]
    lists = rx.ring_lists(index, counts, rings)
    for got, want in zip(lists, want_lists):
        assert got.tolist() == want
        assert np.all(np.diff(got.astype(np.int64)) > 0)           # ascending
    assert sorted(np.concatenate(lists).tolist()) == list(range(n))   # a partition of range(n)


@pytest.mark.parametrize("case,rings,rr_start", _params())
def test_cursor_carried_across_a_split(case, rings, rr_start):
    """The batch cut in two at any point, the cursor carried: the ring ids of the unsplit run."""
    hashes, ok = golden_io.flow_hash(case)
    n = len(hashes)
    ring, _, counts, rr_next = rx.dispatch_host(hashes, ok, rings, rr_start)
    # the cursor a cut carries, in closed form: the start plus the fallbacks before the cut
    miss_before = np.concatenate([[0], np.cumsum(~ok.astype(bool))])
    # every cut for the short cases and, for the long ones, at rings 4 from cursor 3 (the other
    # ring counts of a long case take every 97th cut and the ends: a cut costs two O(n) calls)
    every = n <= 1200 or (rings, rr_start) == (4, 3)
    cuts = range(n + 1) if every else list(range(0, n + 1, 97)) + [1, n - 1, n]
    for cut in cuts:
        a = rx.dispatch_host(hashes[:cut], ok[:cut], rings, rr_start)
        assert a[3] == (rr_start + int(miss_before[cut])) & (rings - 1)
        b = rx.dispatch_host(hashes[cut:], ok[cut:], rings, a[3])
        assert np.array_equal(np.concatenate([a[0], b[0]]), ring), cut
        assert b[3] == rr_next
        assert np.array_equal(a[2] + b[2], counts)


def test_rings_argument():
    h, ok = np.zeros(4, np.uint32), np.ones(4, bool)
    for bad in (0, 3, 128, -2):
        with pytest.raises(ValueError):
            rx.dispatch_host(h, ok, bad, 0)
    ring, index, counts, rr = rx.dispatch_host(h[:0], ok[:0], 4, 3)
    assert ring.size == 0 and index.size == 0 and counts.tolist() == [0] * 5 and rr == 3


def test_a_parsed_packet_hashing_to_zero_is_not_a_fallback():
    ring, index, counts, rr = rx.dispatch_host(np.array([0, 7, 0], np.uint32),
                                               np.array([True, False, True]), 4, 2)
    assert ring.tolist() == [0, 2 | rx.FALLBACK, 0] and rr == 3
    assert index.tolist() == [0, 2, 1] and counts.tolist() == [2, 0, 1, 0, 1]


def test_constants_match_the_header_and_the_binding():
    from upe_amd import gpu

    src = open(os.path.join(ROOT, "include", "upe_gpu.h")).read()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\w+)", src).group(1).rstrip("u"), 0)

    assert define("UPE_RX_RINGS_MAX") == rx.RINGS_MAX == gpu.RX_RINGS_MAX
    assert define("UPE_RX_FALLBACK") == rx.FALLBACK == gpu.RX_FALLBACK
    assert define("UPE_RX_BLOCK") == gpu.RX_BLOCK
    assert "upe_gpu_rx_dispatch" in gpu.EXPORTED and hasattr(gpu.LIB, "upe_gpu_rx_dispatch")
    assert callable(gpu.GpuWorker.rx_dispatch)

"""The RX thread's dispatch of packets to the worker rings, restated on the host with numpy
(reference src/rx_pcap.c:19-25,67-80): a packet whose parse_flow_key succeeds goes to ring
flow_hash & (rings - 1); every other packet (ARP and ICMPv6 NS/NA among them) to the ring the
round-robin cursor names, and the cursor steps; each ring receives its packets in arrival order.
This is the expected value of upe_gpu_rx_dispatch in the tests and the host comparison of
tools/rx_dispatch_time.py.  Ring-full drops (src/rx_pcap.c:31-36) and the 32-packet staging bursts
are host ring mechanics and not modelled."""
from __future__ import annotations

import numpy as np

RINGS_MAX = 64          # UPE_RX_RINGS_MAX
FALLBACK = 0x80000000   # UPE_RX_FALLBACK


def dispatch_host(hashes, ok, rings: int, rr_start: int = 0):
    """(ring, index, counts, rr_next) for one batch.

    hashes, ok: flow_hash per packet and whether parse_flow_key succeeded (golden_io.flow_hash).
    ring:   uint32 per packet, the ring id, | FALLBACK where the cursor chose it.
    index:  uint32, the stable partition by ring: ring r's packets, ascending, are
            index[counts[:r].sum() : counts[:r + 1].sum()].
    counts: uint64[rings + 1], packets per ring, then the number of fallback packets.
    rr_next: the cursor for the next batch, (rr_start + counts[rings]) & (rings - 1)."""
    if rings <= 0 or rings & (rings - 1) or rings > RINGS_MAX:
        raise ValueError("rings must be a power of two between 1 and 64")
    h = np.asarray(hashes, np.uint32)
    ok = np.asarray(ok).astype(bool)
    mask = np.uint32(rings - 1)
    miss = ~ok
    # the k-th fallback packet (k from 0) finds the cursor at rr_start + k
    turn = (np.uint32(rr_start) & mask) + (np.cumsum(miss, dtype=np.uint32) - np.uint32(1))
    rid = np.where(ok, h & mask, turn & mask).astype(np.uint32)
    index = np.argsort(rid, kind="stable").astype(np.uint32)
    counts = np.zeros(rings + 1, np.uint64)
    counts[:rings] = np.bincount(rid, minlength=rings)
    counts[rings] = int(miss.sum())
    ring = np.where(miss, rid | np.uint32(FALLBACK), rid).astype(np.uint32)
    return ring, index, counts, int((rr_start + int(counts[rings])) & (rings - 1))


def ring_lists(index, counts, rings: int):
    """The per-ring packet lists of a dispatch: index cut at the rings' starts."""
    ends = np.cumsum(np.asarray(counts[:rings], np.int64))
    return [index[int(e - c):int(e)] for e, c in zip(ends, np.asarray(counts[:rings], np.int64))]

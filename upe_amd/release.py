"""The order in which the reference worker releases a classified batch's buffers, in numpy:
upe_gpu_release_order (include/upe_gpu.h, csrc/upe_release.hip) and upe_release_order_host
(csrc/upe_host.c) give the same bytes.

worker_main (reference src/worker.c:280-303) frees a packet that is not forwarded at its exit from
process_packet, in packet order, and the forwarded ones — tx_bufs[] — after the burst's
tx_send_batch, in queue order.  Per burst [s, e) with r packets whose verdict code is not FWD:
order[s : s + r] are those packets, order[s + r : e] the forwarded ones, each ascending.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .layout import RELEASE_INFO_DTYPE, TX_BATCH_MAX, V_CONSUMED, V_FWD, VF_ARP_REPLY

RELEASE_BLOCK = 1024      # UPE_RELEASE_BLOCK: packets per workgroup of the kernels
NONE64 = 0xFFFFFFFFFFFFFFFF


class Release(NamedTuple):
    """order, handle, burst_fwd and reply are None where the call writes nothing: all four when
    info.bad_bursts is nonzero, handle without a slot array."""
    order: np.ndarray | None       # n uint32
    handle: np.ndarray | None      # n uint32: slot[order]
    burst_fwd: np.ndarray | None   # one uint32 per burst
    reply: np.ndarray | None       # info.replies uint32
    info: np.ndarray               # RELEASE_INFO_DTYPE record


def fixed_first(n: int, burst: int) -> np.ndarray:
    """The offset array of bursts of a fixed size: nb + 1 uint32."""
    return np.append(np.arange(0, n, burst, dtype=np.uint32), np.uint32(n))


def bad_bursts(first: np.ndarray, n: int) -> int:
    """The violated conditions of an offset array: first[0] == 0, first[nb] == n, every burst 1 to
    TX_BATCH_MAX packets (the difference taken modulo 2^32, as the device takes it)."""
    f = np.asarray(first, np.uint32)
    size = (f[1:] - f[:-1] - np.uint32(1)).astype(np.uint32)
    return int(f[0] != 0) + int(f[-1] != n) + int((size >= TX_BATCH_MAX).sum())


def order_host(verdict: np.ndarray, first: np.ndarray | None = None, burst: int | None = None,
               slot: np.ndarray | None = None) -> Release:
    """upe_release_order_host in numpy.  Exactly one of first (nb + 1 ascending offsets) and burst
    (a fixed size, 1..TX_BATCH_MAX) describes the bursts."""
    assert (first is None) != (burst is None), "bursts: an offset array or a fixed size"
    v = np.asarray(verdict, np.uint32)
    n = len(v)
    code = v & np.uint32(0xF)
    fwd = code == V_FWD
    rep = np.nonzero(v & np.uint32(VF_ARP_REPLY))[0]
    info = np.zeros(1, RELEASE_INFO_DTYPE)[0]
    info["packets"] = n
    info["forwarded"] = int(fwd.sum())
    info["consumed"] = int((code == V_CONSUMED).sum())
    info["dropped"] = n - int(info["forwarded"]) - int(info["consumed"])
    info["replies"] = len(rep)
    info["first_reply"] = int(rep[0]) if len(rep) else NONE64
    if n == 0:
        z = np.zeros(0, np.uint32)
        return Release(z, None if slot is None else z, z, z, info)
    if first is None:
        assert 1 <= burst <= TX_BATCH_MAX
        f = fixed_first(n, burst)
    else:
        f = np.asarray(first, np.uint32)
        assert 1 <= len(f) - 1 <= n
        info["bad_bursts"] = bad_bursts(f, n)
    info["bursts"] = len(f) - 1
    if info["bad_bursts"]:
        return Release(None, None, None, None, info)
    f = f.astype(np.int64)
    size = np.diff(f)
    i = np.arange(n, dtype=np.int64)
    s = np.repeat(f[:-1], size)                    # the first packet of each packet's burst
    other = np.cumsum(~fwd) - ~fwd                 # packets not forwarded before each packet
    before = other - other[s]                      # ... within its burst
    r = np.add.reduceat((~fwd).astype(np.int64), f[:-1])
    pos = np.where(fwd, s + np.repeat(r, size) + (i - s - before), s + before)
    order = np.empty(n, np.uint32)
    order[pos] = i
    handle = None if slot is None else np.asarray(slot, np.uint32)[order]
    return Release(order, handle, (size - r).astype(np.uint32), rep.astype(np.uint32), info)

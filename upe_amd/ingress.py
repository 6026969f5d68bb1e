"""The ingress batch of a burst of pktbuf handles, restated on the host with numpy: the frames of
the buffers the handles name (a pool of stride-byte buffers: timestamp@0, len@8, data@16; the
reference's pktbuf_t with stride 2064, include/pktbuf.h:8-14) as the "Batch layout" the classify
calls take — in place (REF), as 96-byte header windows (WINDOW) or packed back to back (FULL) —
plus the buffers' timestamps, the positions of the packets that may write a neighbour table and
the summary (the rules of upe_gpu_ingress_gather, include/upe_gpu.h).  This is the expected value
of upe_gpu_ingress_gather in the tests and the host comparison of tools/ingress_gather_time.py."""
from __future__ import annotations

import numpy as np

from .layout import HDR_WINDOW, INGRESS_INFO_DTYPE, make_desc

REF, WINDOW, FULL = 0, 1, 2       # UPE_INGRESS_REF / _WINDOW / _FULL
NONE = 0xFFFFFFFFFFFFFFFF         # first_bad / first_ctrl when there is none


def _spread(starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """The byte positions starts[k] .. starts[k] + lens[k] - 1 of every k, concatenated."""
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(total, dtype=np.int64)


def table_writes(data: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """Per frame: may handle_control_packet write a neighbour table (is_table_write in
    upe_worker.c)?  data: (n, >= 55) uint8, row k = frame k's first bytes; bytes at or past
    lens[k] read as zero."""
    d = np.where(np.arange(55)[None, :] < lens[:, None], data[:, :55], 0).astype(np.int64)
    et = d[:, 12] << 8 | d[:, 13]
    arp = (et == 0x0806) & np.all(d[:, 14:20] == np.array([0, 1, 8, 0, 6, 4]), axis=1)
    nd = (et == 0x86DD) & (lens >= 78) & (d[:, 20] == 58) & ((d[:, 54] == 135) | (d[:, 54] == 136))
    return arp | nd


def gather_host(pool, stride, slots, mode, out_bytes=None):
    """(out, desc, timestamps, ctrl, info) for one burst.

    pool:   uint8, the pool's bytes (pool_bytes = its size); buffer s is pool[s*stride:(s+1)*stride].
    slots:  the handles' buffer indexes in arrival order.  A handle is bad when its buffer does not
            lie inside the pool, or its 64-bit len exceeds stride - 16 or 65535: it keeps its
            position with a descriptor of len 0, no bytes (FULL), a zero window (WINDOW), no mark;
            its timestamp is the buffer's, or 0 for a slot outside the pool.
    mode:   REF (out empty, descriptors relative to the pool), WINDOW (96 bytes per packet) or FULL
            (the packing rule of egress.pack_host).
    out_bytes: the output's capacity (None: whatever is needed).  WINDOW needs n * 96 (ValueError
            otherwise, the call's -1).  FULL: frame k, at offset o_k = the sum of the padded lengths
            before it, is written only if o_k + padded_k <= out_bytes.
    out:    uint8[info.bytes]; desc / timestamps: info.packed entries; ctrl: the marked positions
            below info.packed, ascending; info: an INGRESS_INFO_DTYPE record, whose bad, first_bad,
            n_ctrl and first_ctrl count all n handles."""
    pool = np.asarray(pool, np.uint8)
    slots = np.asarray(slots, np.uint32).astype(np.int64)
    stride = int(stride)
    if mode not in (REF, WINDOW, FULL):
        raise ValueError("unknown ingress mode")
    if stride % 16 or stride < 16 + 96 or not stride <= pool.size <= 1 << 36:
        raise ValueError("bad stride or pool size")
    n = slots.size
    info = np.zeros(1, INGRESS_INFO_DTYPE)[0]
    info["packets"] = n
    inside = slots < pool.size // stride
    base = np.where(inside, slots, 0) * stride
    head = pool[base[:, None] + np.arange(16)].view("<u8").reshape(n, 2)
    ts = np.where(inside, head[:, 0], np.uint64(0))
    bad = ~inside | (head[:, 1] > np.uint64(min(stride - 16, 65535)))
    lens = np.where(bad, np.uint64(0), head[:, 1]).astype(np.int64)
    first = pool[base[:, None] + 16 + np.arange(55)]   # stride >= 112: inside the buffer
    marks = table_writes(first, lens)
    info["bad"], info["n_ctrl"] = np.count_nonzero(bad), np.count_nonzero(marks)
    info["first_bad"] = np.nonzero(bad)[0][0] if bad.any() else NONE
    info["first_ctrl"] = np.nonzero(marks)[0][0] if marks.any() else NONE
    packed = n
    if mode == REF:
        out = np.zeros(0, np.uint8)
        desc = make_desc(np.where(bad, 16, base + 16), lens)
    elif mode == WINDOW:
        if out_bytes is not None and out_bytes < n * HDR_WINDOW:
            raise ValueError("the output is smaller than n header windows")
        out = np.zeros(n * HDR_WINDOW, np.uint8)
        wl = np.minimum(lens, HDR_WINDOW)
        out[_spread(np.arange(n, dtype=np.int64) * HDR_WINDOW, wl)] = pool[_spread(base + 16, wl)]
        desc = make_desc(np.arange(n, dtype=np.int64) * HDR_WINDOW, lens)
        info["bytes"] = info["need"] = out.size
    else:
        padded = (lens + 15) & ~np.int64(15)
        ends = np.cumsum(padded)
        need = int(ends[-1]) if n else 0
        cap = need if out_bytes is None else int(out_bytes)
        packed = int(np.count_nonzero(ends <= cap))   # ends ascend: a prefix
        used = int(ends[packed - 1]) if packed else 0
        starts = (ends - padded)[:packed]
        out = np.zeros(used, np.uint8)
        out[_spread(starts, lens[:packed])] = pool[_spread(base[:packed] + 16, lens[:packed])]
        desc = make_desc(np.where(bad[:packed], 16, starts), lens[:packed])
        info["bytes"], info["need"] = used, need
    info["packed"] = packed
    ctrl = np.nonzero(marks[:packed])[0].astype(np.uint32)
    return out, desc, ts[:packed].astype(np.uint64), ctrl, info


def make_pool(frames, lens, slots, capacity, stride, timestamps=None, fill=0):
    """A pool of `capacity` stride-byte buffers, every byte `fill`, with frames[k] (uint8; may be
    longer than lens[k]: the surplus is stale data in the buffer) written into buffer slots[k],
    whose len field is lens[k] (any 64-bit value) and whose timestamp is timestamps[k] (default
    k + 1).  Returns the pool's bytes (uint8[capacity * stride])."""
    pool = np.full(capacity * stride, fill, np.uint8)
    head = np.zeros(2, "<u8")
    for k, (f, s) in enumerate(zip(frames, slots)):
        f = np.asarray(f, np.uint8)
        assert 0 <= s < capacity and f.size <= stride - 16
        head[0] = k + 1 if timestamps is None else timestamps[k]
        head[1] = lens[k]
        at = int(s) * stride
        pool[at:at + 16] = head.view(np.uint8)
        pool[at + 16:at + 16 + f.size] = f
    return pool

"""The neighbour-table writes of a batch's control packets, restated on the host with numpy: the
records handle_control_packet (reference src/worker.c:23-104) would hand to arp_update /
ndp_update, in packet order, and those two table functions (src/arp_table.c:26-53,
src/ndp_table.c:39-65 from hash_ipv6 :6-17) over the slot arrays.  This is the expected value of
upe_gpu_ctrl_writes, upe_ctrl_writes_host and upe_neigh_apply_writes (include/upe_gpu.h) in the
tests.  It needs no GPU and no library: the walk and the probes are written straight from the
reference's statements."""
from __future__ import annotations

import numpy as np

from .ingress import table_writes
from .layout import (ARP_DTYPE, CTRL_INFO_DTYPE, CTRL_WRITE_DTYPE, CW_ARP, CW_NDP, NDP_DTYPE,
                     desc_lens, desc_offsets)

NONE = 0xFFFFFFFFFFFFFFFF   # first_write when the batch has no record
CTRL_BLOCK = 1024           # UPE_CTRL_BLOCK


def marks(frames: np.ndarray, desc: np.ndarray) -> np.ndarray:
    """Per packet: may handle_control_packet write a neighbour table (ctrl_table_write,
    csrc/upe_dev.h; the rule of upe_gpu_ingress_gather's d_ctrl)?  Bytes at or past len read as
    zero."""
    frames = np.asarray(frames, np.uint8)
    offs, lens = desc_offsets(desc), desc_lens(desc)
    if len(offs) == 0:
        return np.zeros(0, bool)
    at = np.minimum(offs[:, None] + np.arange(55), frames.size - 1)   # masked by len below
    return table_writes(frames[at], lens)


def record(f: np.ndarray, index: int):
    """The record of one marked frame f (its len bytes), or None: an NS / NA none of whose
    options the walk of src/worker.c:68-95 accepts."""
    ln = len(f)
    at = lambda j: int(f[j]) if j < ln else 0   # noqa: E731  (a zero-filled pktbuf)
    w = np.zeros(1, CTRL_WRITE_DTYPE)[0]
    w["index"] = index
    if at(12) == 0x08:
        # src/worker.c:34-35: arp_update(ntohl(spa), sha); the learn does not look at len
        w["kind"], w["mac_off"] = CW_ARP, 22
        w["mac"] = [at(22 + j) for j in range(6)]
        spa = at(28) << 24 | at(29) << 16 | at(30) << 8 | at(31)
        w["ip"][:4] = np.frombuffer(spa.to_bytes(4, "little"), np.uint8)
        return w
    ns = f[54] == 135
    off = 78
    while off + 2 <= ln:
        ot, ol = int(f[off]), (int(f[off + 1]) * 8) & 0xFF   # uint8_t opt_len: 32 wraps to 0
        if ol == 0 or off + ol > ln:
            break
        if (ns and ot == 1) or (not ns and ot == 2):
            w["kind"], w["mac_off"] = CW_NDP, off + 2
            w["mac"] = f[off + 2:off + 8]
            w["ip"] = f[22:38] if ns else f[62:78]
            return w
        off += ol
    return None


def ctrl_writes(frames, desc, cap=None):
    """(writes, info): the batch's records as a CTRL_WRITE_DTYPE array — the first min(writes,
    cap) of them, in packet order (cap None: all) — and the CTRL_INFO_DTYPE record."""
    frames = np.asarray(frames, np.uint8)
    desc = np.asarray(desc, np.uint64)
    if len(desc) > 0xFFFFFFFF - CTRL_BLOCK:
        raise ValueError("n must fit in 32 bits")
    offs, lens = desc_offsets(desc), desc_lens(desc)
    marked = np.nonzero(marks(frames, desc))[0]
    recs = []
    for i in marked:
        r = record(frames[offs[i]:offs[i] + lens[i]], int(i))
        if r is not None:
            recs.append(r)
    info = np.zeros(1, CTRL_INFO_DTYPE)[0]
    info["ctrl"], info["writes"] = len(marked), len(recs)
    info["first_write"] = recs[0]["index"] if recs else NONE
    keep = len(recs) if cap is None else min(len(recs), int(cap))
    info["stored"] = keep
    out = np.zeros(keep, CTRL_WRITE_DTYPE)
    for k in range(keep):
        out[k] = recs[k]
    return out, info


def _slot(valid, same, home, cap):
    """The slot arp_update / ndp_update writes: from `home`, the first that is free or holds the
    address; None after `cap` probes (a full table of other addresses is left alone)."""
    for k in range(cap):
        s = (home + k) & (cap - 1)
        if not valid[s] or same(s):
            return s
    return None


def apply_writes(arp, ndp, writes, now: int) -> int:
    """arp_update / ndp_update of each record, in order, on the slot arrays (ARP_DTYPE /
    NDP_DTYPE, power-of-two lengths, in place; None or empty: no table of that family), with
    update_at = now on every slot written.  Returns the records whose family has a table.
    Everything is checked before the first write (ValueError)."""
    arp = np.zeros(0, ARP_DTYPE) if arp is None else arp
    ndp = np.zeros(0, NDP_DTYPE) if ndp is None else ndp
    writes = np.asarray(writes, CTRL_WRITE_DTYPE)
    for t, dt in ((arp, ARP_DTYPE), (ndp, NDP_DTYPE)):
        if t.dtype != dt or len(t) & (len(t) - 1):
            raise ValueError("a slot array of the table's dtype, its capacity a power of two")
    if not np.isin(writes["kind"], (CW_ARP, CW_NDP)).all():
        raise ValueError("a record's kind is neither CW_ARP nor CW_NDP")
    applied = 0
    for w in writes:
        if w["kind"] == CW_ARP:
            t = arp
            if len(t) == 0:
                continue
            ip = int(w["ip"][:4].view("<u4")[0])
            s = _slot(t["valid"], lambda s: int(t["ip"][s]) == ip, ip, len(t))
            new = ip
        else:
            t = ndp
            if len(t) == 0:
                continue
            ip = w["ip"].copy()
            home = int(np.bitwise_xor.reduce(ip.view("<u4")))
            s = _slot(t["valid"], lambda s: np.array_equal(t["ip"][s], ip), home, len(t))
            new = ip
        applied += 1
        if s is None:
            continue
        if not t["valid"][s]:
            t["valid"][s] = 1
            t["ip"][s] = new
        t["mac"][s] = w["mac"]
        t["update_at"][s] = now
    return applied

"""The egress batch of a classified batch, restated on the host with numpy: the forwarded frames
(verdict code UPE_V_FWD) as process_packet leaves them in b->data, in the order the reference
queues them for tx_send_batch (src/worker.c:240-243, 287-303), back to back at 16-byte aligned
offsets with zeroed padding, plus their descriptors and ingress indexes (the packing rule of
upe_gpu_egress_pack, include/upe_gpu.h).  This is the expected value of upe_gpu_egress_pack in
the tests and the host comparison of tools/egress_pack_time.py."""
from __future__ import annotations

import numpy as np

from .layout import EGRESS_INFO_DTYPE, V_FWD, desc_lens, desc_offsets, make_desc


def _spread(starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """The byte positions starts[k] .. starts[k] + lens[k] - 1 of every k, concatenated."""
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(total, dtype=np.int64)


def pack_host(frames, desc, verdict, hdr=None, out_bytes=None):
    """(out, out_desc, out_index, info) for one classified batch.

    frames, desc, verdict: the ingress batch ("Batch layout") and its verdict words; only the
            verdict code is read.
    hdr:    None when the frames were rewritten in place; else the emit-mode records as the device
            holds them, (n, 16) uint8 in the UPE_HDR_SLOT layout (forwarded packet i's record at
            64 * (i // 64) + its rank among the forwarded packets of its 64-group), applied to the
            untouched frames by upe_hdr_apply's byte rule; a patched position at or beyond a
            frame's length is not written.
    out_bytes: the output's capacity (None: whatever is needed).  Frame k, at offset o_k = the sum
            of the padded lengths before it, is packed only if o_k + padded_k <= out_bytes.
    out:    uint8[info.bytes]; out_desc / out_index: info.packed entries;
    info:   an EGRESS_INFO_DTYPE record (frames, packed, bytes, need)."""
    frames = np.asarray(frames, np.uint8)
    desc = np.asarray(desc, np.uint64)
    v = np.asarray(verdict, np.uint32)
    is_fwd = (v & np.uint32(0xF)) == V_FWD
    fwd = np.nonzero(is_fwd)[0]
    lens, offs = desc_lens(desc)[fwd], desc_offsets(desc)[fwd]
    padded = (lens + 15) & ~np.int64(15)
    ends = np.cumsum(padded)
    need = int(ends[-1]) if fwd.size else 0
    cap = need if out_bytes is None else int(out_bytes)
    packed = int(np.count_nonzero(ends <= cap))   # ends ascend: a prefix
    used = int(ends[packed - 1]) if packed else 0
    fwd, lens, offs = fwd[:packed], lens[:packed], offs[:packed]
    starts = (ends - padded)[:packed]
    out = np.zeros(used, np.uint8)
    out[_spread(starts, lens)] = frames[_spread(offs, lens)]
    if hdr is not None and packed:
        # UPE_HDR_SLOT: the rank of a forwarded packet inside its 64-group
        f = is_fwd.astype(np.int64)
        excl = np.cumsum(f) - f
        grp = fwd & ~np.int64(63)
        rec = np.asarray(hdr, np.uint8).reshape(-1, 16)[grp + excl[fwd] - excl[grp]]
        fam = rec[:, 15]
        # upe_hdr_apply (src/worker.c:174-176, 197-200, 213, 227-230 as bytes)
        puts = [(fam == 4) | (fam == 6)] * 12 + [fam == 4, fam == 4, fam == 4, fam == 6]
        where = list(range(12)) + [22, 24, 25, 21]
        which = list(range(12)) + [12, 13, 14, 12]
        for m, pos, b in zip(puts, where, which):
            m = m & (lens > pos)
            out[starts[m] + pos] = rec[m, b]
    info = np.zeros(1, EGRESS_INFO_DTYPE)[0]
    info["frames"], info["packed"], info["bytes"], info["need"] = (
        int(np.count_nonzero(is_fwd)), packed, used, need)
    return out, make_desc(starts, lens), fwd.astype(np.uint32), info

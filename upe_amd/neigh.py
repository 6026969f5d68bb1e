"""arp_get_mac and ndp_get_mac restated on the host with numpy, over arrays of flow keys (reference
src/arp_table.c:55-80, src/ndp_table.c:67-86 from hash_ipv6 :6-17).  This is the expected value of
upe_gpu_resolve_keys and upe_neigh_lookup_host in the tests and the host side of
tools/resolve_keys_time.py.  It needs no GPU and no library: the probe is written straight from the
reference's statements, over the slot arrays themselves — no index is built.

Every key probes at once: step i looks at slot (home + i) & (capacity - 1) of the keys still
probing; a key leaves with the slot's MAC where the slot is valid and holds its address, and with
nothing where the slot is invalid.  After `capacity` steps whoever is left has seen every slot."""
from __future__ import annotations

import numpy as np

from .layout import ARP_DTYPE, FLOW_KEY_DTYPE, NDP_DTYPE

MAC_FOUND = 1 << 48   # UPE_MAC_FOUND (include/upe_gpu.h)


def _mac_words(mac: np.ndarray) -> np.ndarray:
    """(slots, 6) MAC bytes -> the answer of a hit: byte 0 lowest, bit 48 set."""
    out = np.full(len(mac), MAC_FOUND, np.uint64)
    for j in range(6):
        out |= mac[:, j].astype(np.uint64) << np.uint64(8 * j)
    return out


def _probe(home: np.ndarray, addr: np.ndarray, slot_addr: np.ndarray, valid: np.ndarray,
           answer: np.ndarray) -> np.ndarray:
    """home: (m,) starting slots before masking; addr: (m, w) addresses asked for; slot_addr:
    (capacity, w), valid: (capacity,) bool, answer: (capacity,) uint64 per slot."""
    out = np.zeros(len(home), np.uint64)
    cap = len(valid)
    if cap == 0 or len(home) == 0:
        return out
    mask = np.uint64(cap - 1)
    live = np.arange(len(home))
    cur = home.astype(np.uint64) & mask
    for _ in range(cap):
        s = cur.astype(np.int64)
        ok = valid[s]
        hit = ok & (slot_addr[s] == addr[live]).all(axis=1)
        out[live[hit]] = answer[s[hit]]
        go = ok & ~hit
        live, cur = live[go], (cur[go] + np.uint64(1)) & mask
        if live.size == 0:
            break
    return out


def resolve_keys(arp, ndp, keys) -> np.ndarray:
    """uint64 per key (FLOW_KEY_DTYPE): ip_ver 4 -> arp_get_mac(dst_ip.v4), the union's bytes 0-3
    as a little-endian word; 6 -> ndp_get_mac(dst_ip.v6); anything else -> not found.  A hit is
    the six MAC bytes in bits 0-47 (byte 0 lowest) with bit 48 set, a miss exactly 0.  arp / ndp:
    the slot arrays (ARP_DTYPE / NDP_DTYPE, power-of-two lengths), or None / empty."""
    arp = np.zeros(0, ARP_DTYPE) if arp is None else np.asarray(arp, ARP_DTYPE)
    ndp = np.zeros(0, NDP_DTYPE) if ndp is None else np.asarray(ndp, NDP_DTYPE)
    keys = np.asarray(keys, FLOW_KEY_DTYPE).ravel()
    for t in (arp, ndp):
        assert len(t) & (len(t) - 1) == 0, "capacity must be a power of two (arp_table_init)"
    out = np.zeros(len(keys), np.uint64)
    dst = np.ascontiguousarray(keys["dst_ip"]).reshape(-1, 16)
    words = dst.view("<u4").reshape(-1, 4)
    is4, is6 = keys["ip_ver"] == 4, keys["ip_ver"] == 6
    # arp_get_mac: idx = ip & (capacity - 1)
    ip = words[is4, 0]
    out[is4] = _probe(ip, ip[:, None], np.ascontiguousarray(arp["ip"])[:, None],
                      arp["valid"] != 0, _mac_words(arp["mac"]))
    # ndp_get_mac: idx = hash_ipv6 = the XOR of the four words as the bytes lie, & (capacity - 1)
    w6 = words[is6]
    home = w6[:, 0] ^ w6[:, 1] ^ w6[:, 2] ^ w6[:, 3] if len(w6) else np.zeros(0, np.uint32)
    slot_words = np.ascontiguousarray(ndp["ip"]).reshape(-1, 16).view("<u4").reshape(-1, 4)
    out[is6] = _probe(home, w6, slot_words, ndp["valid"] != 0, _mac_words(ndp["mac"]))
    return out


_M32 = 0xFFFFFFFF


def slots3(k: int, seed: int, bits: int):
    """slot1 / slot2 / slot3 of csrc/upe_dev.h: an index key's three candidate slots."""
    s1 = (((k ^ seed) * 0x9E3779B1) & _M32) >> (32 - bits)
    x = ((k ^ seed) * 0x85EBCA77) & _M32
    s2 = (((x ^ (x >> 16)) * 0xC2B2AE3D) & _M32) >> (32 - bits)
    x = ((k ^ ((seed * 0x9E3779B9) & _M32)) * 0x27D4EB2F) & _M32
    s3 = (((x ^ (x >> 15)) * 0x165667B1) & _M32) >> (32 - bits)
    return s1, s2, s3


def fold_v6(w) -> int:
    """fold_v6 of csrc/upe_dev.h: the NDP index's key of an address's four little-endian words."""
    return (((w[0] * 0x9E3779B1) & _M32) ^ ((w[1] * 0x85EBCA77) & _M32) ^
            ((w[2] * 0xC2B2AE3D) & _M32) ^ ((w[3] * 0x27D4EB2F) & _M32))


def _update(t, home: int, same, ip, mac) -> None:
    """arp_update / ndp_update (reference src/arp_table.c:26-53, src/ndp_table.c:39-65): from the
    home slot, the first slot that is invalid or holds the address takes it; a full table without
    it is left alone.  update_at is not modelled."""
    cap = len(t)
    for j in range(cap):
        s = (home + j) & (cap - 1)
        if not t["valid"][s] or same(s):
            t["ip"][s], t["mac"][s], t["valid"][s] = ip, mac, 1
            return


def learn(index, writes, arp=None, ndp=None):
    """upe_gpu_neigh_learn restated: the contract's loop (include/upe_gpu.h) over the records
    (CTRL_WRITE_DTYPE, in rank order) on the index — (info, arp_slots, ndp_slots) as
    gpu.NeighImage.read() gives it: the NEIGH_IMAGE_INFO_DTYPE record and the slot arrays as uint32
    words — and, where they are given, arp_update / ndp_update of every record that is not deferred
    on the slot arrays the index was compiled from.  Returns (index, defer, info, arp, ndp): the
    changed copies, the deferred ranks ascending (uint32) and (records, patched, inserted, dropped,
    deferred, first_defer, arp_free, ndp_free), first_defer 2^64 - 1 where nothing is deferred."""
    meta, aslots, nslots = index
    meta, aslots, nslots = meta.copy(), aslots.copy(), nslots.copy()
    arp = None if arp is None else np.asarray(arp, ARP_DTYPE).copy()
    ndp = None if ndp is None else np.asarray(ndp, NDP_DTYPE).copy()
    w = np.asarray(writes).ravel()
    free = {4: int(meta["arp_free"]), 6: int(meta["ndp_free"])}
    counts = [0, 0, 0]   # patched, inserted, dropped
    defer = []
    for r in range(len(w)):
        kind = int(w["kind"][r])
        if kind not in (4, 6):
            defer.append(r)
            continue
        v6 = kind == 6
        fam = "ndp" if v6 else "arp"
        bits, seed = int(meta[fam + "_bits"]), int(meta[fam + "_seed"])
        slots = nslots if v6 else aslots
        words = [int(x) for x in np.frombuffer(w["ip"][r].tobytes(), "<u4")]
        if not v6:
            words = words[:1]
        mac = w["mac"][r].tobytes()
        lo, hi = int.from_bytes(mac[:4], "little"), int.from_bytes(mac[4:], "little")
        used_at, mac_at = (5, 4) if v6 else (2, 1)   # the word with the used bit; the MAC's first
        cand = slots3(fold_v6(words) if v6 else words[0], seed, bits) if bits else ()
        hit = [c for c in cand if (slots[c, used_at] >> 16) & 1 and
               [int(x) for x in slots[c, :len(words)]] == words]
        outcome = None
        if hit:
            c = hit[0]
            slots[c, mac_at] = lo
            slots[c, mac_at + 1] = (int(slots[c, mac_at + 1]) & 0xFFFF0000) | hi
            outcome = 0
        elif not int(meta[fam + "_insertable"]):
            defer.append(r)
        elif free[kind] == 0:
            outcome = 2
        else:
            room = [c for c in cand if not (slots[c, used_at] >> 16) & 1]
            if not room:
                defer.append(r)
            else:
                slots[room[0]] = 0
                slots[room[0], :len(words)] = words
                slots[room[0], mac_at] = lo
                slots[room[0], mac_at + 1] = hi | 1 << 16
                free[kind] -= 1
                outcome = 1
        if outcome is None:
            continue
        counts[outcome] += 1
        t = ndp if v6 else arp
        if t is not None and len(t):
            ip = w["ip"][r] if v6 else words[0]
            if v6:
                x = words[0] ^ words[1] ^ words[2] ^ words[3]
                _update(t, x, lambda s: t["ip"][s].tobytes() == w["ip"][r].tobytes(), ip, w["mac"][r])
            else:
                _update(t, words[0], lambda s: int(t["ip"][s]) == words[0], ip, w["mac"][r])
    meta["arp_free"], meta["ndp_free"] = free[4], free[6]
    first = defer[0] if defer else (1 << 64) - 1
    info = (len(w), counts[0], counts[1], counts[2], len(defer), first, free[4], free[6])
    return (meta, aslots, nslots), np.asarray(defer, np.uint32), info, arp, ndp


def patch(arp, ndp, writes):
    """upe_gpu_neigh_patch restated on the slot arrays: the records (CTRL_WRITE_DTYPE, in rank
    order) whose address the probe above reaches before the batch — arp_get_mac of ip bytes 0-3 for
    kind 4, ndp_get_mac of the 16 bytes for kind 6 — rewrite the MAC of the slot that answers, the
    last one aimed at a slot staying; every other record (an address no probe reaches, a family
    without slots, another kind) is missed and changes nothing.  A refresh moves nothing, so
    "reached before the batch" is "reached when the record's turn comes".  update_at is not
    modelled.  Returns (arp, ndp, miss, info): patched copies of the arrays, the missed records'
    ranks ascending (uint32), and (records, patched, missed, first_miss), first_miss 2^64 - 1
    where nothing is missed."""
    arp = (np.zeros(0, ARP_DTYPE) if arp is None else np.asarray(arp, ARP_DTYPE)).copy()
    ndp = (np.zeros(0, NDP_DTYPE) if ndp is None else np.asarray(ndp, NDP_DTYPE)).copy()
    w = np.asarray(writes).ravel()
    n = len(w)
    ip = np.ascontiguousarray(w["ip"]).reshape(n, 16)
    words = ip.view("<u4").reshape(n, 4)
    is4, is6 = w["kind"] == 4, w["kind"] == 6
    # the slot that answers, as the probe's answer: slot + 1, 0 = not reached
    slot = np.zeros(n, np.uint64)
    a4 = words[is4, 0]
    slot[is4] = _probe(a4, a4[:, None], np.ascontiguousarray(arp["ip"])[:, None],
                       arp["valid"] != 0, np.arange(1, len(arp) + 1, dtype=np.uint64))
    w6 = words[is6]
    home = w6[:, 0] ^ w6[:, 1] ^ w6[:, 2] ^ w6[:, 3] if len(w6) else np.zeros(0, np.uint32)
    slot_words = np.ascontiguousarray(ndp["ip"]).reshape(-1, 16).view("<u4").reshape(-1, 4)
    slot[is6] = _probe(home, w6, slot_words, ndp["valid"] != 0,
                       np.arange(1, len(ndp) + 1, dtype=np.uint64))
    held = slot != 0
    # in rank order: numpy's fancy assignment keeps the last of equal indexes
    for t, fam in ((arp, is4), (ndp, is6)):
        r = np.nonzero(fam & held)[0]
        if len(r):
            t["mac"][(slot[r] - 1).astype(np.int64)] = w["mac"][r]
    miss = np.nonzero(~held)[0].astype(np.uint32)
    first = int(miss[0]) if len(miss) else (1 << 64) - 1
    return arp, ndp, miss, (n, n - len(miss), len(miss), first)

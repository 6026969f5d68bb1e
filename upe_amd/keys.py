"""parse_flow_key and rule_table_match restated on the host with numpy, over arrays (reference
src/parser.c:6-111; src/rule_table.c:163-176 over match_rule :76-91).  This is the expected value
of upe_gpu_parse_keys and upe_gpu_match_keys in the tests and the host side of
tools/match_keys_time.py.  It needs no GPU and no library: both functions are written straight
from the reference's statements, gate by gate and field by field."""
from __future__ import annotations

import numpy as np

from .layout import FLOW_KEY_DTYPE, RULE_DTYPE

WINDOW = 96   # the parser reads no byte past 14 + 60 + 13 (an IPv4 TCP header's data offset)


def parse_keys(frames, desc):
    """(keys, rc) of a batch in the batch layout (frames: uint8, desc: offset << 16 | len).

    keys: FLOW_KEY_DTYPE per packet, what parse_flow_key leaves in a key zeroed beforehand; all
          44 bytes zero where the parse fails.
    rc:   int32 per packet, 0 or -1.
    A byte at or past a frame's len is never looked at (it reads as zero, as in a zero-filled
    pktbuf, and every gate that passes has checked the bytes it uses lie below len)."""
    frames = np.ascontiguousarray(frames, np.uint8).ravel()
    desc = np.asarray(desc, np.uint64).ravel()
    n = len(desc)
    keys = np.zeros(n, FLOW_KEY_DTYPE)
    if n == 0:
        return keys, np.zeros(0, np.int32)
    off = (desc >> np.uint64(16)).astype(np.int64)
    ln = (desc & np.uint64(0xFFFF)).astype(np.int64)
    col = np.arange(WINDOW, dtype=np.int64)
    below = col[None, :] < ln[:, None]
    if frames.size:
        at = np.minimum(off[:, None] + col[None, :], frames.size - 1)
        w = np.where(below, frames[at], 0).astype(np.int64)
    else:
        w = np.zeros((n, WINDOW), np.int64)
    rows = np.arange(n)
    eth = ln >= 14                                               # parser.c:8-10
    et = (w[:, 12] << 8) | w[:, 13]
    ip_len = ln - 14
    vihl = w[:, 14]
    hl = (vihl & 0xF) * 4
    ok4 = eth & (et == 0x0800) & (ip_len >= 20) & ((vihl >> 4) == 4) & (hl >= 20) & (ip_len >= hl)
    ok6 = eth & (et == 0x86DD) & (ip_len >= 40)                  # parser.c:46-64
    proto = np.where(ok4, w[:, 23], np.where(ok6, w[:, 20], 0))
    l4_off = np.where(ok4, 14 + hl, 54)
    l4_len = np.where(ok4, ip_len - hl, ip_len - 40)

    def l4(k):
        return w[rows, np.minimum(l4_off + k, WINDOW - 1)]

    def be16(k):
        return (l4(k) << 8) | l4(k + 1)

    thl = (l4(12) >> 4) * 4
    udp = (proto == 17) & (l4_len >= 8)                          # parser.c:70-78
    tcp = (proto == 6) & (l4_len >= 20) & (thl >= 20) & (l4_len >= thl)   # parser.c:79-94
    icmp = (proto == 1) & (l4_len >= 8)                          # parser.c:95-105
    ok = (ok4 | ok6) & (udp | tcp | icmp)
    g4, g6 = ok & ok4, ok & ok6
    keys["ip_ver"] = np.where(g4, 4, np.where(g6, 6, 0))
    # IPv4: ntohl of the wire word, stored as a host (little-endian) uint32: the bytes reversed
    keys["src_ip"][g4, :4] = w[g4, 26:30][:, ::-1]
    keys["dst_ip"][g4, :4] = w[g4, 30:34][:, ::-1]
    keys["src_ip"][g6] = w[g6, 22:38]
    keys["dst_ip"][g6] = w[g6, 38:54]
    keys["protocol"] = np.where(ok, proto, 0)
    keys["src_port"] = np.where(ok, np.where(icmp, be16(4), be16(0)), 0)    # icmp: id
    keys["dst_port"] = np.where(ok, np.where(icmp, be16(0), be16(2)), 0)    # type << 8 | code
    return keys, np.where(ok, 0, -1).astype(np.int32)


def match_keys(rules_sorted, keys):
    """int32 per key: the index in rules_sorted (the table's (priority, rule_id) order) of the
    first rule match_rule accepts, or -1: no rule does, or the key's ip_ver is neither 4 nor 6
    (upe_rules_match_host's convention; match_rule would skip the address test for such a key, and
    parse_flow_key never produces one).  Of an IPv4 key's addresses only union bytes 0-3 count."""
    rules = np.ascontiguousarray(rules_sorted, RULE_DTYPE)
    k = np.ascontiguousarray(keys, FLOW_KEY_DTYPE)
    out = np.full(len(k), -1, np.int32)
    todo = np.nonzero((k["ip_ver"] == 4) | (k["ip_ver"] == 6))[0]
    ver = k["ip_ver"]
    used = np.arange(16)[None, :] < np.where(ver == 4, 4, 16)[:, None]   # address bytes compared
    for i, r in enumerate(rules):
        if todo.size == 0:
            break
        m = np.ones(todo.size, bool)
        if r["ip_ver"]:
            m &= ver[todo] == r["ip_ver"]
        if r["protocol"]:
            m &= k["protocol"][todo] == r["protocol"]
        if r["src_port"]:
            m &= k["src_port"][todo] == r["src_port"]
        if r["dst_port"]:
            m &= k["dst_port"][todo] == r["dst_port"]
        for ip, mask, kip in ((r["src_ip"], r["src_mask"], k["src_ip"]),
                              (r["dst_ip"], r["dst_mask"], k["dst_ip"])):
            diff = (kip[todo] ^ ip[None, :]) & mask[None, :]
            m &= ~np.any((diff != 0) & used[todo], axis=1)
        out[todo[m]] = i
        todo = todo[~m]
    return out

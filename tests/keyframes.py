"""Frames from flow keys: the inverse of parse_flow_key (reference src/parser.c:6-111), so that
a test can aim traffic at a rule table key by key (the rules' own edges, one-bit near misses)
and still send it through the whole path as well-formed packets.

A key is TCP, UDP or ICMP over IPv4 or IPv6.  ICMP (protocol 1) is kept: the parser takes it
under either ethertype (src/parser.c:95-105 tests the protocol byte alone), reads the identifier
into src_port and type << 8 | code into dst_port, so every 16-bit pair can be produced exactly.
An IPv4 key carries only bytes 0-3 of its address fields (host order); the parser leaves the
rest zero, as canonical() does.
"""
from __future__ import annotations

import numpy as np

from upe_amd import synth
from upe_amd.layout import FLOW_KEY_DTYPE

RUN = 64   # packets per wave: the matchers are templated on "some lane holds IPv6"


def canonical(keys: np.ndarray) -> np.ndarray:
    """The keys as parse_flow_key writes them: an IPv4 key's address bytes 4-15 zero."""
    out = np.zeros(len(keys), FLOW_KEY_DTYPE)
    for f in FLOW_KEY_DTYPE.names:
        out[f] = keys[f]
    v4 = out["ip_ver"] == 4
    out["src_ip"][v4, 4:] = 0
    out["dst_ip"][v4, 4:] = 0
    return out


def arrange_runs(keys: np.ndarray) -> np.ndarray:
    """The same keys ordered so that the batch holds whole 64-packet runs of IPv4 only, then of
    IPv6 only (a quarter of each family's keys, rounded down to whole runs), then the rest in
    their given order, mixed packet by packet."""
    is6 = keys["ip_ver"] == 6
    i4, i6 = np.nonzero(~is6)[0], np.nonzero(is6)[0]
    n4 = len(i4) // 4 // RUN * RUN
    n6 = len(i6) // 4 // RUN * RUN
    rest = np.sort(np.concatenate([i4[n4:], i6[n6:]]))
    return keys[np.concatenate([i4[:n4], i6[:n6], rest])]


def run_kinds(keys: np.ndarray) -> set:
    """Which kinds of aligned 64-packet run the batch holds: "v4", "v6", "mixed"."""
    is6 = keys["ip_ver"] == 6
    kinds = set()
    for s in range(0, len(keys) - RUN + 1, RUN):
        c = int(is6[s:s + RUN].sum())
        kinds.add("v4" if c == 0 else "v6" if c == RUN else "mixed")
    return kinds


def frames_from_keys(keys: np.ndarray, rng) -> tuple[np.ndarray, np.ndarray]:
    """(frames, desc) in the batch layout, frame i parsing to canonical(keys)[i].  IPv4 headers
    have IHL 5, a tenth 6-15 (the general path); TCP data offset 5, a tenth 6-10; TTL and hop
    limit 2-128 (a forwarded packet is never dropped for its TTL); lengths 64-200, never
    shorter than the headers."""
    keys = canonical(keys)
    n = len(keys)
    ver, proto = keys["ip_ver"], keys["protocol"].astype(np.int64)
    if not (np.isin(ver, [4, 6]).all() and np.isin(proto, [1, 6, 17]).all()):
        raise ValueError("keys must be TCP, UDP or ICMP over IPv4 or IPv6")
    sport, dport = keys["src_port"].astype(np.uint32), keys["dst_port"].astype(np.uint32)
    h = np.zeros((n, 128), np.uint8)
    synth._macs(h, rng)
    ttl = rng.integers(2, 129, size=n)
    doff = np.where(rng.random(n) < 0.1, rng.integers(6, 11, size=n), 5)
    ihl = np.where(rng.random(n) < 0.1, rng.integers(6, 16, size=n), 5)
    ihl = np.where(ver == 4, ihl, 0)
    l3 = np.where(ver == 4, 14 + 4 * ihl, 54)
    hdr_len = l3 + np.where(proto == 6, 4 * doff, 8)
    lens = np.maximum(rng.integers(64, 201, size=n), hdr_len)
    r4, r6 = np.nonzero(ver == 4)[0], np.nonzero(ver == 6)[0]
    if len(r4):
        addr = lambda f: np.ascontiguousarray(keys[f][r4, :4]).view("<u4").ravel().astype(np.uint64)
        synth.build_ipv4(h, r4, src=addr("src_ip"), dst=addr("dst_ip"), proto=proto[r4],
                         ttl=ttl[r4], ihl=ihl[r4], total_len=lens[r4] - 14,
                         l4_ports=(sport[r4], dport[r4]), tcp_doff=doff[r4],
                         icmp=(dport[r4] >> 8, dport[r4] & 0xFF, sport[r4]), rng=rng)
    if len(r6):
        synth.build_ipv6(h, r6, src16=keys["src_ip"][r6], dst16=keys["dst_ip"][r6], nh=proto[r6],
                         hop=ttl[r6], payload_len=lens[r6] - 54, sport=sport[r6], dport=dport[r6],
                         tcp_doff=doff[r6])
        ic = r6[proto[r6] == 1]   # ICMP header: type, code, checksum, identifier
        h[ic, 54] = dport[ic] >> 8
        h[ic, 55] = dport[ic] & 0xFF
        h[ic, 56:58] = 0
        h[ic, 58] = sport[ic] >> 8
        h[ic, 59] = sport[ic] & 0xFF
    return synth.pack_frames(h, lens)

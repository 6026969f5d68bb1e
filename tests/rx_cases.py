"""Chosen batches for the RX dispatch (upe_gpu_rx_dispatch, upe_amd/rx.py): every packet's ring
is decided by the case, not by a traffic draw.  No GPU; the oracle library gives the hashes.

pool()          a small fixed frame buffer and one descriptor per frame.  For every ring id r in
                0..63 four frames that parse (UDP/IPv4, TCP/IPv4, ICMP/IPv4, UDP/IPv6) with seeded
                addresses and far port, the source port (ICMP: the id) solved so that the
                reference's flow_hash & 63 == r; then FALLBACKS frames parse_flow_key rejects, each
                for another reason.  A batch is a descriptor array that aliases the pool, so a
                million packets cost 8 MB of descriptors and no frame building.
pool_hashes()   the reference's parse result and flow_hash per pool frame (oracle.parse +
                upe_ref_flow_hash): what a batch's expected values are gathered from.
assignment()    (kind, ring) per packet for a pattern: PARSED to a chosen ring, or FALLBACK.
batch()         an assignment as (desc, hashes, ok); which of a ring's frames a parsed packet
                takes (ring ids that agree modulo `rings`, four variants each) and which fallback
                frame are seeded draws.
closed_form()   the dispatch of three patterns written out by hand, without rx.dispatch_host.

SMALL sits on the wave (64), workgroup (256) and tile (BLOCK) edges and on the step from 8 to 9
tiles, where the scan's second lane and the padded column stride start to matter; LARGE on the
scan's step of 512 tiles: ragged and full, the first tile of a second step, the second step's
second lane, and a third step.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import oracle
from upe_amd import synth
from upe_amd.layout import FRAME_TAIL, make_desc

BLOCK = 1024        # UPE_RX_BLOCK: packets per tile
SCAN_STEP = 512     # tiles per step of the scan: 64 lanes x 8 tiles
RING_IDS = 64       # UPE_RX_RINGS_MAX
RINGS = (1, 2, 4, 8, 16, 32, 64)
VARIANTS = ("udp4", "tcp4", "icmp4", "udp6")
FALLBACKS = ("runt", "arp", "icmp6_ns", "ip4_proto47", "udp4_cut")
PARSED, FALLBACK = 0, 1
PATTERNS = ("one_ring", "lane_ring", "wave_ring", "tile_ring", "all_fallback", "first_fallback",
            "last_fallback", "edge_fallback", "alternate", "runs", "seeded")
LARGE_PATTERNS = ("seeded", "all_fallback", "tile_ring", "runs")
RUNS = (1, 63, 64, 65, 1023, 1025)
SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4097, 8191, 8192, 8193, 9216)
LARGE = (511 * 1024 + 1023, 512 * 1024, 512 * 1024 + 1, 520 * 1024 + 5, 1024 * 1024 + 1)


def rr_starts(rings: int):
    """The three cursors every case starts from (fewer where they coincide)."""
    return sorted({0, rings - 1, 0x7FFFFFF3 & (rings - 1)})


# ---- the pool ----------------------------------------------------------------------------------

def ref_hash(frame: bytes, length: int | None = None):
    """(parse_flow_key succeeded, flow_hash) of one frame, from the oracle library."""
    rc, key = oracle.parse(frame, length)
    if rc != 0:
        return False, 0
    return True, int(oracle.oracle_lib().upe_ref_flow_hash(key.ctypes.data_as(ctypes.c_void_p)))


def _parsing_frame(variant: str, r: int, rng) -> bytes:
    """A frame of the variant whose flow_hash & 63 is r.  flow_hash is an XOR over the key's
    fields, so the solved field is r folded into the hash the frame has with that field zero;
    the field's upper ten bits are drawn."""
    a4, b4 = (int(x) for x in rng.integers(1, 1 << 32, 2))
    a6, b6 = (bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(2))
    other = int(rng.integers(0, 1 << 16))
    hi = int(rng.integers(0, 1 << 10)) << 6

    def build(x: int) -> bytes:
        if variant == "udp4":
            return synth._frame(synth._eth(0x0800), synth._ip4(17, a4, b4), synth._udp(x, other))
        if variant == "tcp4":
            return synth._frame(synth._eth(0x0800), synth._ip4(6, a4, b4), synth._tcp(x, other))
        if variant == "icmp4":   # the id is the key's sport, type << 8 | code its dport
            return synth._frame(synth._eth(0x0800), synth._ip4(1, a4, b4),
                                synth._icmp(other >> 8, other & 0xFF, x))
        assert variant == "udp6"
        return synth._frame(synth._eth(0x86DD), synth._ip6(17, a6, b6, plen=8),
                            synth._udp(x, other))

    ok, h0 = ref_hash(build(0))
    assert ok, variant
    return build(hi | ((h0 ^ r) & 63))


def _fallback_frames():
    """(name, frame bytes, len): each fails parse_flow_key at another gate."""
    v6a = bytes.fromhex("20010db80000000000000000000000a1")
    v6b = bytes.fromhex("20010db80000000000000000000000b2")
    mac = bytes.fromhex("0a1b2c3d4e5f")
    udp = synth._frame(synth._eth(0x0800), synth._ip4(17, 0x0A000001, 0x0A800005),
                       synth._udp(1000, 53))
    out = {
        "runt": (bytes(range(1, 11)), 10),                                   # len < 14
        "arp": (synth._frame(synth._eth(0x0806, dst=b"\xff" * 6),            # the ethertype
                             synth._arp(1, mac, 0xC0A80A07, bytes(6), 0x0A800001)), None),
        "icmp6_ns": (synth._frame(synth._eth(0x86DD), synth._ip6(58, v6a, v6b, plen=32),
                                  bytes([135, 0, 0, 0, 0, 0, 0, 0]) + v6b,
                                  bytes([1, 1]) + mac), None),               # protocol 58
        "ip4_proto47": (synth._frame(synth._eth(0x0800), synth._ip4(47, 0x0A000005, 0x0A80000A),
                                     synth._udp(1, 2)), None),               # an unknown protocol
        "udp4_cut": (udp, len(udp) - 1),                                     # 7 of the 8 L4 bytes
    }
    assert tuple(out) == FALLBACKS
    return [(k, f, len(f) if ln is None else ln) for k, (f, ln) in out.items()]


@functools.lru_cache(maxsize=None)
def pool_items():
    """[(name, frame bytes, len)]: frame 4 * r + v is variant v of ring id r, then the fallbacks."""
    rng = np.random.default_rng(0x5258)
    items = []
    for r in range(RING_IDS):
        for v in VARIANTS:
            f = _parsing_frame(v, r, rng)
            items.append((f"{v} ring {r}", f, len(f)))
    return items + _fallback_frames()


@functools.lru_cache(maxsize=None)
def pool():
    """(frames, desc): every frame whole (a cut frame keeps the bytes past its len) at a 16-byte
    boundary, FRAME_TAIL readable bytes behind the last one."""
    items = pool_items()
    sizes = np.array([max(len(f), 16) for _, f, _ in items], np.int64)
    slots = (sizes + 15) & ~np.int64(15)
    offs = np.cumsum(slots) - slots
    frames = np.zeros(int(slots.sum()) + FRAME_TAIL, np.uint8)
    for (_, f, _), o in zip(items, offs):
        frames[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    desc = make_desc(offs, np.array([ln for _, _, ln in items], np.int64))
    frames.setflags(write=False)
    desc.setflags(write=False)
    return frames, desc


@functools.lru_cache(maxsize=None)
def pool_hashes():
    """(hashes uint32, ok bool) per pool frame, from the reference's parse and hash."""
    got = [ref_hash(f, ln) for _, f, ln in pool_items()]
    ok = np.array([k for k, _ in got], bool)
    hashes = np.array([h for _, h in got], np.uint32)
    ok.setflags(write=False)
    hashes.setflags(write=False)
    return hashes, ok


# ---- assignments -------------------------------------------------------------------------------

def tile_edges(n: int) -> np.ndarray:
    """The last packet of every tile that has a successor, and the first of the next."""
    first = np.arange(BLOCK, n, BLOCK, dtype=np.int64)
    return np.sort(np.concatenate([first - 1, first]))


def _seed(tag: int, n: int, rings: int, pattern: str):
    return np.random.default_rng([tag, n, rings, PATTERNS.index(pattern)])


def assignment(n: int, rings: int, pattern: str):
    """(kind uint8[n], ring int32[n]): packet i is PARSED to ring[i], or a FALLBACK (ring -1)."""
    assert n > 0 and rings in RINGS
    i = np.arange(n, dtype=np.int64)
    fb = np.zeros(n, bool)
    lane = i % rings
    if pattern == "one_ring":
        ring = np.full(n, rings - 1, np.int64)
    elif pattern == "lane_ring":
        ring = lane
    elif pattern == "wave_ring":
        ring = (i // 64) % rings
    elif pattern == "tile_ring":
        ring = (i // BLOCK) % rings
    elif pattern == "all_fallback":
        ring, fb[:] = lane, True
    elif pattern == "first_fallback":
        ring, fb[0] = lane, True
    elif pattern == "last_fallback":
        ring, fb[-1] = lane, True
    elif pattern == "edge_fallback":
        ring = (i // 64) % rings
        fb[tile_edges(n)] = True
    elif pattern == "alternate":
        ring, fb = lane, (i & 1) == 1
    elif pattern == "runs":
        # alternating fallback and parsed runs; the lengths are drawn without replacement, six
        # at a time, so every length is there from sum(RUNS) packets on; a parsed packet's ring
        # is drawn
        rng = _seed(1, n, rings, pattern)
        draws = n // sum(RUNS) + 1
        ends = np.cumsum(rng.permuted(np.tile(RUNS, (draws, 1)), axis=1).ravel())
        fb = ((np.searchsorted(ends, i, side="right") + int(rng.integers(0, 2))) & 1) == 1
        ring = rng.integers(0, rings, n)
    elif pattern == "seeded":
        # half the parsed packets on ring 0, the rest uniform; about one packet in ten a fallback
        rng = _seed(1, n, rings, pattern)
        fb = rng.random(n) < 0.10
        ring = np.where(rng.random(n) < 0.5, 0, rng.integers(0, rings, n))
    else:
        raise ValueError(pattern)
    return (np.where(fb, FALLBACK, PARSED).astype(np.uint8),
            np.where(fb, -1, ring).astype(np.int32))


def batch(n: int, rings: int, pattern: str):
    """(desc, hashes, ok) of the pattern's batch over pool()'s frames.  A packet parsed to ring q
    takes a frame of a ring id that is q modulo `rings` (so the mask cuts real bits) in one of
    the four variants; hashes and ok are the pool's reference values, not derived from ring[]."""
    kind, ring = assignment(n, rings, pattern)
    rng = _seed(2, n, rings, pattern)
    rid = ring.astype(np.int64) + rings * rng.integers(0, RING_IDS // rings, n)
    fid = np.where(kind == PARSED, 4 * rid + rng.integers(0, len(VARIANTS), n),
                   RING_IDS * len(VARIANTS) + rng.integers(0, len(FALLBACKS), n))
    hashes, ok = pool_hashes()
    return pool()[1][fid], hashes[fid], ok[fid]


# ---- closed forms ------------------------------------------------------------------------------

def closed_form(n: int, rings: int, pattern: str, rr: int):
    """(ring, index, counts) of the pattern's dispatch from cursor rr, written out by hand."""
    i = np.arange(n, dtype=np.uint32)
    counts = np.zeros(rings + 1, np.uint64)
    if pattern == "all_fallback":
        # the cursor alone: packet i to ring (rr + i) & (rings - 1), each ring every rings-th
        rid = (np.uint32(rr & (rings - 1)) + i) & np.uint32(rings - 1)
        lists = [i[(r - rr) % rings::rings] for r in range(rings)]
        ring = rid | np.uint32(0x80000000)
        counts[rings] = n
    elif pattern == "one_ring":
        lists = [i[:0]] * (rings - 1) + [i]
        ring = np.full(n, rings - 1, np.uint32)
    elif pattern == "tile_ring":
        # ring r's list: the whole tiles r, r + rings, ... one after another
        tiles = [i[t:t + BLOCK] for t in range(0, n, BLOCK)]
        lists = [np.concatenate(tiles[r::rings] or [i[:0]]) for r in range(rings)]
        ring = (i // np.uint32(BLOCK)) % np.uint32(rings)
    else:
        raise ValueError(pattern)
    counts[:rings] = [len(x) for x in lists]
    return ring.astype(np.uint32), np.concatenate(lists).astype(np.uint32), counts


CLOSED = ("all_fallback", "one_ring", "tile_ring")

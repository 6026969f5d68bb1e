"""The gate matrix: every truncation of every header shape, in buffers whose bytes at or past a
frame's length are not zero.

include/upe_gpu.h promises "Bytes at or beyond a frame's length are never used", and the device
parsers keep that promise by masking (they load whole 16-byte quads).  synth.pack_frames writes
min(len, width) bytes of each frame into a zeroed buffer, so in every other batch of the suite a
gate that forgot its length test still reads zeros.  Here every slot is filled first (zero as the
control, 0xFF, the shape's own untruncated bytes, or random bytes) and the frame's first `len`
bytes written over it: under the `parent` fill a truncated frame looks complete to any reader
that goes past `len`.

matrix(fill, order)       -> (Workload, parent_len, shape_id, is_truncated): the whole matrix
boundary_subset(fill)     -> the same for the frames within one byte of a gate (at most 1024)
control_subset(fill)      -> the ARP / NS / NA shapes with all truncations, each followed by probe
                             packets to the address it teaches (at most 1024 frames)
SHAPES                    -> the shapes (name, bytes, kind, IHL, ...), indexed by shape_id

Shapes (synth._eth / _ip4 / _ip6 / _udp / _tcp / _icmp / _arp; two payload bytes behind the L4
header): IPv4 with IHL 5..15 x {UDP, TCP doff 5, TCP doff 15, ICMP} with seeded option bytes, one
UDP shape per IHL with options 0xFF, id 0xFFFF and total length 0xFFFF (the checksum fold carries
as often as it can); IPv6 x {UDP, TCP doff 5, TCP doff 8, ICMP as protocol 1, ICMPv6 echo, NS with
SLLA, NA with TLLA}; four ARP shapes with four bytes of padding (an answered request cut
inside bytes 42..47 must keep the buffer's own bytes there).  Each of these appears at every
length 0..full.  Single full-length frames: IHL 0..4, a version nibble other than 4, TCP data
offsets 0..4, TTL / hop limit 0, 1, 2, a VLAN tag, ethertype 0x88CC, protocols 0, 47, 50, 58 and
255 over IPv4.

Rules: one exact FWD rule per parsing shape (distinct addresses and ports per shape, so a field
taken from the wrong place misses its rule), two DROP rules, a rule with an unknown action type, a
version-0 rule, wildcard FWD rules for the control subset's probes and a catch-all DROP at
priority 9999.  The catch-all is IPv4's: a version-agnostic one would leave UPE_V_DROP_NOMATCH
unreachable, and tests/test_gate_matrix.py requires every verdict code.  Six more single frames
(`probe_*`) exist only to reach the rules no shape of the list above reaches: both DROP rules, the
unknown action, the version-0 rule from either family, and no rule at all.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from upe_amd import synth
from upe_amd.layout import ACT_DROP, ACT_FWD, FRAME_TAIL, make_desc
from upe_amd.synth import _arp, _eth, _frame, _icmp, _ip4, _ip6, _tcp, _udp

STRIDE = 256            # bytes per slot: every frame starts at a multiple of it
FILLS = ("zero", "ones", "parent", "random")
ORDERS = ("grouped", "shuffled")
MAX_FRAMES = 16384
MAX_SUBSET = 1024
PROBE_PORT = 4789       # destination port of the control subset's probes (wildcard FWD rules)

SEED_SHAPES, SEED_FILL, SEED_ORDER, SEED_RULES = 7301, 7302, 7303, 7304

MAC_SRC = bytes.fromhex("0a0b0c0d0e0f")


def _v6(prefix: str, k: int) -> bytes:
    return bytes.fromhex(prefix) + bytes(8) + k.to_bytes(2, "big")


@dataclasses.dataclass(frozen=True)
class Shape:
    name: str
    data: bytes
    multi: bool              # appears at every length 0..len(data); else once, whole
    family: int = 0          # 4 / 6 for IP shapes, 0 otherwise
    l4: str = ""             # "udp", "tcp5", "tcp15", "tcp8", "icmp", "ff" (UDP, all-ones options), ...
    ihl: int = 0
    min_parse: int = 0       # the least len at which parse_flow_key succeeds (0: it never does)
    key: tuple | None = None  # (ip_ver, proto, src, dst, sport, dport) of a parsing shape
    control: str = ""        # "arp", "ns", "na"
    teaches: object = None   # the address a control shape teaches (int v4 or bytes v6)


def _build_shapes():
    rng = np.random.default_rng(SEED_SHAPES)
    shapes: list[Shape] = []
    k4 = 0
    pay = b"\xc3\x3c"

    def v4_flow():
        nonlocal k4
        k = k4
        k4 += 1
        return 0x0A010000 + 0x0101 * (k + 1), 0x0A800100 + k, 1000 + 2 * k, 2001 + 2 * k, 3000 + k

    # ---- IPv4, IHL 5..15 x L4 kind, every length ----
    for ihl in range(5, 16):
        for l4 in ("udp", "tcp5", "tcp15", "icmp", "ff"):
            src, dst, sp, dp, ident = v4_flow()
            n_opt = ihl * 4 - 20
            if l4 == "ff":
                ip = bytearray(_ip4(17, src, dst, ihl=ihl, total=0xFFFF, opts=b"\xff" * n_opt))
                ip[4:6] = b"\xff\xff"                                   # id
                ip = bytes(ip)
            else:
                proto = {"udp": 17, "tcp5": 6, "tcp15": 6, "icmp": 1}[l4]
                opts = bytes(rng.integers(0, 256, n_opt, dtype=np.uint8))
                ip = _ip4(proto, src, dst, ihl=ihl, total=ihl * 4 + 10, opts=opts)
            if l4 in ("udp", "ff"):
                body, key, l4len = _udp(sp, dp), (4, 17, src, dst, sp, dp), 8
            elif l4 == "icmp":
                body, key, l4len = _icmp(8, 0, ident), (4, 1, src, dst, ident, 0x0800), 8
            else:
                doff = 5 if l4 == "tcp5" else 15
                body, key, l4len = _tcp(sp, dp, doff=doff), (4, 6, src, dst, sp, dp), 4 * doff
            data = _frame(_eth(0x0800), ip, body, pay)
            shapes.append(Shape(f"v4_ihl{ihl}_{l4}", data, True, 4, l4, ihl,
                                14 + 4 * ihl + l4len, key))

    # ---- IPv6, every length ----
    k6 = 0

    def v6_flow():
        nonlocal k6
        k6 += 1
        return _v6("20010db80001", 0x100 + k6), _v6("2001db800002", k6), 5000 + 2 * k6, 6001 + 2 * k6

    for l4 in ("udp", "tcp5", "tcp8", "icmp", "echo", "ns", "na"):
        src, dst, sp, dp = v6_flow()
        key, control, teaches, mp = None, "", None, 0
        if l4 == "udp":
            nh, body, key, mp = 17, _udp(sp, dp), (6, 17, src, dst, sp, dp), 62
        elif l4 in ("tcp5", "tcp8"):
            doff = int(l4[3:])
            nh, body, key, mp = 6, _tcp(sp, dp, doff=doff), (6, 6, src, dst, sp, dp), 54 + 4 * doff
        elif l4 == "icmp":
            nh, body, key, mp = 1, _icmp(8, 0, sp), (6, 1, src, dst, sp, 0x0800), 62
        elif l4 == "echo":
            nh, body = 58, bytes([128, 0, 0, 0]) + sp.to_bytes(2, "big") + b"\x00\x01"
        elif l4 == "ns":      # teaches (ip6.src, SLLA)
            nh, control, teaches = 58, "ns", src
            body = bytes([135, 0, 0, 0, 0, 0, 0, 0]) + dst + bytes([1, 1]) + bytes.fromhex("5a5b5c5d5e01")
        else:                 # NA teaches (target, TLLA)
            target = _v6("20010db80003", 0x77)
            nh, control, teaches = 58, "na", target
            body = bytes([136, 0, 0, 0, 0x60, 0, 0, 0]) + target + bytes([2, 1]) + \
                bytes.fromhex("5a5b5c5d5e02")
        data = _frame(_eth(0x86DD), _ip6(nh, src, dst, plen=len(body) + 2), body, pay)
        shapes.append(Shape(f"v6_{l4}", data, True, 6, l4, 0, mp, key, control, teaches))

    # ---- ARP, every length ----
    arps = [("arp_req_port", 1, bytes.fromhex("5a5b5c5d5e11"), 0x0A800201, synth.PORT_IP4, 6),
            ("arp_req_other", 1, bytes.fromhex("5a5b5c5d5e12"), 0x0A800202, 0x0A800001, 6),
            ("arp_reply", 2, bytes.fromhex("5a5b5c5d5e13"), 0x0A800203, synth.PORT_IP4, 6),
            ("arp_req_hlen8", 1, bytes.fromhex("5a5b5c5d5e14"), 0x0A800204, synth.PORT_IP4, 8)]
    for name, op, sha, spa, tpa, hlen in arps:
        tha = MAC_SRC if op == 2 else bytes(6)
        data = _frame(_eth(0x0806, dst=b"\xff" * 6 if op == 1 else b"\x02\x00\x00\x00\x00\x01"),
                      _arp(op, sha, spa, tha, tpa, hlen=hlen), pay, pay)
        shapes.append(Shape(name, data, True, control="arp", teaches=spa))

    # ---- single full-length frames ----
    def single(name, data, **kw):
        shapes.append(Shape(name, data, False, **kw))

    def v4_single(proto, body, **kw):
        src, dst, _, _, _ = v4_flow()
        return _frame(_eth(0x0800), _ip4(proto, src, dst, **kw), body, pay)

    for ihl in range(0, 5):
        f = bytearray(v4_single(17, _udp(7, 8)))
        f[14] = 0x40 | ihl
        single(f"v4_ihl{ihl}", bytes(f), family=4)
    single("v4_version6", v4_single(17, _udp(7, 8), ver=6), family=4)
    for doff in range(0, 5):
        f = bytearray(v4_single(6, _tcp(9, 10)))
        f[34 + 12] = doff << 4
        single(f"v4_tcp_doff{doff}", bytes(f), family=4)
    u4 = next(s for s in shapes if s.name == "v4_ihl5_udp")
    u6 = next(s for s in shapes if s.name == "v6_udp")
    for ttl in (0, 1, 2):
        f = bytearray(u4.data)
        f[22] = ttl
        single(f"v4_ttl{ttl}", bytes(f), family=4, key=u4.key)
        f = bytearray(u6.data)
        f[21] = ttl
        single(f"v6_hop{ttl}", bytes(f), family=6, key=u6.key)
    single("vlan", _frame(_eth(0x8100), b"\x00\x01\x08\x00", _ip4(17, 0x0A090901, 0x0A800301),
                          _udp(1, 2), pay))
    single("lldp", _frame(_eth(0x88CC), bytes(rng.integers(0, 256, 40, dtype=np.uint8))))
    for proto in (0, 47, 50, 58, 255):
        single(f"v4_proto{proto}", v4_single(proto, _udp(11, 12)), family=4)

    # ---- frames that exist to reach the rules no shape above reaches (see the module text) ----
    single("probe_drop4", _frame(_eth(0x0800), _ip4(17, 0x0A0A0A01, 0x0A800401), _udp(7001, 7002), pay),
           family=4, key=(4, 17, 0x0A0A0A01, 0x0A800401, 7001, 7002))
    s6, d6 = _v6("20010db80004", 1), _v6("2001db800004", 2)
    single("probe_drop6", _frame(_eth(0x86DD), _ip6(6, s6, d6, plen=22), _tcp(7003, 7004), pay),
           family=6, key=(6, 6, s6, d6, 7003, 7004))
    single("probe_action", _frame(_eth(0x0800), _ip4(1, 0x0A0A0A02, 0x0A800402), _icmp(0, 0, 7005), pay),
           family=4, key=(4, 1, 0x0A0A0A02, 0x0A800402, 7005, 0))
    # the version-0 rule's address bytes 0a 80 00 08 ..: an IPv4 packet compares them as the
    # little-endian word 0x0800800A (8.0.128.10), an IPv6 packet as its first five bytes
    single("probe_ver0_v4", _frame(_eth(0x0800), _ip4(17, 0x0A0A0A03, 0x0800800A), _udp(7006, 7007), pay),
           family=4, key=(4, 17, 0x0A0A0A03, 0x0800800A, 7006, 7007))
    d0 = bytes.fromhex("0a80000800") + bytes(10) + b"\x09"
    single("probe_ver0_v6", _frame(_eth(0x86DD), _ip6(17, s6, d0, plen=10), _udp(7008, 7009), pay),
           family=6, key=(6, 17, s6, d0, 7008, 7009))
    single("probe_nomatch", _frame(_eth(0x86DD), _ip6(17, s6, d6, plen=10), _udp(7010, 7011), pay),
           family=6, key=(6, 17, s6, d6, 7010, 7011))
    assert max(len(s.data) for s in shapes) <= STRIDE - 16
    return tuple(shapes)


SHAPES = _build_shapes()
SHAPE_ID = {s.name: i for i, s in enumerate(SHAPES)}
PARSING = tuple(i for i, s in enumerate(SHAPES) if s.multi and s.key is not None)


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------

def _rule_for(prio, action, key):
    ver, proto, src, dst, sp, dp = key
    plen = 32 if ver == 4 else 128
    return synth.make_rule(prio, action, ip_ver=ver, proto=proto, sport=sp, dport=dp,
                           src=(src, plen), dst=(dst, plen))


@functools.lru_cache(maxsize=None)
def rules() -> np.ndarray:
    """The matrix's table, in a seeded insertion order (the (priority, rule_id) sort matters)."""
    rs = [_rule_for(100 + j, ACT_FWD, SHAPES[i].key) for j, i in enumerate(PARSING)]
    key = {s.name: s.key for s in SHAPES if not s.multi and s.key is not None}
    rs += [_rule_for(20, ACT_DROP, key["probe_drop4"]),
           _rule_for(21, ACT_DROP, key["probe_drop6"]),
           synth.make_rule(30, 2, ip_ver=4, proto=1, sport=7005),            # unknown action type
           synth.make_rule(40, ACT_FWD, ip_ver=0, dst=(bytes.fromhex("0a800008") + bytes(12), 40)),
           synth.make_rule(50, ACT_FWD, ip_ver=4, proto=17, dport=PROBE_PORT),
           synth.make_rule(51, ACT_FWD, ip_ver=6, proto=17, dport=PROBE_PORT),
           synth.make_rule(9999, ACT_DROP, ip_ver=4)]                        # IPv4's catch-all
    order = np.random.default_rng(SEED_RULES).permutation(len(rs))
    out = synth.rules_array([rs[i] for i in order])
    out.setflags(write=False)
    return out


CAPACITY = 128


def _mac(tag: int, k: int) -> bytes:
    return bytes([0x02, tag, 0xCC, 0xDD, k >> 8, k & 0xFF])


def neigh_tables():
    """Every other parsing shape's destination is in its family's table; the rest miss."""
    a = [(SHAPES[i].key[3], _mac(0xA4, i)) for i in PARSING[::2] if SHAPES[i].family == 4]
    n = [(SHAPES[i].key[3], _mac(0xA6, i)) for i in PARSING[::2] if SHAPES[i].family == 6]
    n.append((SHAPES[SHAPE_ID["v6_udp"]].key[3], _mac(0xA6, SHAPE_ID["v6_udp"])))
    return synth.arp_table(256, a), synth.ndp_table(16, n)


def start_l1() -> np.ndarray:
    """Starting L1 entries that name a destination of each family with a MAC the table does not
    hold: the first packets to it take this MAC, the later ones the table's (the look-back)."""
    l1 = synth.l1_zero()
    l1["last_arp_ip"] = SHAPES[SHAPE_ID["v4_ihl5_udp"]].key[3]
    l1["last_arp_mac"] = np.frombuffer(bytes.fromhex("0badc0ffee04"), np.uint8)
    l1["last_ndp_ip"] = np.frombuffer(SHAPES[SHAPE_ID["v6_udp"]].key[3], np.uint8)
    l1["last_ndp_mac"] = np.frombuffer(bytes.fromhex("0badc0ffee06"), np.uint8)
    return l1


# ---------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------

def pack(items, fill: str, seed: int = SEED_FILL):
    """items: (frame bytes, len, parent bytes) triples -> (frames, desc).  Every slot of STRIDE
    bytes, and FRAME_TAIL bytes behind the last one, is filled completely; then the frame's first
    len bytes are written."""
    if fill not in FILLS:
        raise ValueError(fill)
    n = len(items)
    total = n * STRIDE + FRAME_TAIL
    rng = np.random.default_rng(seed)
    if fill == "zero":
        buf = np.zeros(total, np.uint8)
    elif fill == "ones":
        buf = np.full(total, 0xFF, np.uint8)
    else:
        buf = rng.integers(0, 256, total, dtype=np.uint8)
    lens = np.zeros(n, np.int64)
    for i, (data, ln, parent) in enumerate(items):
        o = i * STRIDE
        if fill == "parent":
            buf[o:o + len(parent)] = np.frombuffer(parent, np.uint8)
        buf[o:o + ln] = np.frombuffer(data[:ln], np.uint8)
        lens[i] = ln
    return buf, make_desc(np.arange(n, dtype=np.int64) * STRIDE, lens)


@functools.lru_cache(maxsize=None)
def _entries():
    """(shape_id, len) of every frame of the matrix, grouped by shape."""
    out = []
    for i, s in enumerate(SHAPES):
        out += [(i, ln) for ln in range(len(s.data) + 1)] if s.multi else [(i, len(s.data))]
    assert len(out) < MAX_FRAMES
    return tuple(out)


def _workload(name, entries, fill, arp, ndp, l1):
    items = [(SHAPES[i].data, ln, SHAPES[i].data) for i, ln in entries]
    frames, desc = pack(items, fill)
    sid = np.array([i for i, _ in entries], np.int64)
    lens = np.array([ln for _, ln in entries], np.int64)
    parent = np.array([len(SHAPES[i].data) for i, _ in entries], np.int64)
    wl = synth.Workload(name, frames, desc, rules().copy(), CAPACITY, arp, ndp, l1=l1)
    return wl, parent, sid, lens < parent


def matrix(fill: str, order: str = "grouped"):
    """(Workload, parent_len, shape_id, is_truncated).  grouped: as generated, whole waves of
    general-path frames with the fast-path-eligible full-length ones among them; shuffled: one
    seeded permutation."""
    if order not in ORDERS:
        raise ValueError(order)
    ent = list(_entries())
    if order == "shuffled":
        ent = [ent[i] for i in np.random.default_rng(SEED_ORDER).permutation(len(ent))]
    arp, ndp = neigh_tables()
    out = _workload(f"gates-{fill}-{order}", ent, fill, arp, ndp, start_l1())
    assert out[0].n < MAX_FRAMES and out[0].frames.nbytes < 4 << 20
    return out


def gate_lengths(s: Shape) -> set[int]:
    """The lengths at which a parser's decision about shape s changes (the first length that
    passes each gate), and those at which a device parser loads another 16-byte quad."""
    full = len(s.data)
    g = {14, full}
    if s.family == 4:
        g |= {34, 14 + 4 * s.ihl}
        if s.min_parse:
            g.add(s.min_parse)
        if s.l4.startswith("tcp"):
            g.add(14 + 4 * s.ihl + 20)
        g |= {49, 65, 81}
    elif s.family == 6:
        g |= {54, 49, 65, 78}
        if s.min_parse:
            g.add(s.min_parse)
        if s.l4.startswith("tcp"):
            g.add(74)
    elif s.control == "arp":
        g |= {20, 42}
    return {x for x in g if 0 <= x <= full}


def boundary_subset(fill: str = "parent"):
    """The frames of the matrix whose length is within one byte of a gate of their shape (and
    every single frame), at most MAX_SUBSET: same tuple as matrix().  The all-ones option shapes
    are left to the whole matrix."""
    ent = []
    for i, ln in _entries():
        s = SHAPES[i]
        if s.l4 == "ff":
            continue
        if not s.multi or any(abs(ln - g) <= 1 for g in _core_gates(s)):
            ent.append((i, ln))
    assert len(ent) <= MAX_SUBSET, len(ent)
    arp, ndp = neigh_tables()
    return _workload(f"gates-boundary-{fill}", ent, fill, arp, ndp, start_l1())


def _core_gates(s: Shape) -> set[int]:
    """gate_lengths without the quad-load lengths a shape's own gates do not need: what fits
    MAX_SUBSET frames.  The 81-byte load is kept where it matters (IHL >= 14 with TCP)."""
    g = gate_lengths(s) - {49, 65, 81}
    if s.family == 4 and s.ihl >= 14 and s.l4.startswith("tcp"):
        g.add(81)
    if s.family == 6 or s.name in ("v4_ihl5_udp", "v4_ihl5_tcp5", "v4_ihl9_tcp15"):
        g |= {x for x in (49, 65) if x <= len(s.data)}
    return g


def control_subset(fill: str = "parent"):
    """Every ARP and NS / NA shape at every length, each followed by two UDP probes to the
    address the whole frame teaches (one probe where the cut lies inside the Ethernet header: no
    reader of such a frame can learn from it, and two probes each would pass MAX_SUBSET).  The
    tables start with one of the taught IPv4 addresses under an older MAC.  Same tuple as
    matrix(); probes carry shape_id -1 and parent_len = their length."""
    items, sid, parent = [], [], []
    k = 0
    for i, s in enumerate(SHAPES):
        if not s.control:
            continue
        k += 1
        if s.control == "arp":
            probe = _frame(_eth(0x0800), _ip4(17, 0x0A090000 + k, s.teaches), _udp(4000 + k, PROBE_PORT),
                           b"\xc3\x3c")
        else:
            probe = _frame(_eth(0x86DD), _ip6(17, _v6("20010db80009", k), s.teaches, plen=10),
                           _udp(4000 + k, PROBE_PORT), b"\xc3\x3c")
        for ln in range(len(s.data) + 1):
            items.append((s.data, ln, s.data))
            sid.append(i)
            parent.append(len(s.data))
            for _ in range(1 if ln < 14 else 2):
                items.append((probe, len(probe), probe))
                sid.append(-1)
                parent.append(len(probe))
    assert len(items) <= MAX_SUBSET, len(items)
    frames, desc = pack(items, fill)
    lens = np.array([ln for _, ln, _ in items], np.int64)
    arp = synth.arp_table(16, [(0x0A800202, bytes.fromhex("02a4ccdd0bad")),
                               (0x0A800105, bytes.fromhex("02a4ccdd0105"))])
    ndp = synth.ndp_table(16, [(_v6("2001db800002", 1), bytes.fromhex("02a6ccdd0001"))])
    wl = synth.Workload(f"gates-control-{fill}", frames, desc, rules().copy(), CAPACITY, arp, ndp)
    parent = np.array(parent, np.int64)
    return wl, parent, np.array(sid, np.int64), lens < parent


def describe(i: int, wl, parent_len, shape_id) -> str:
    """shape, len and parent_len of frame i, for assertion messages."""
    sid = int(shape_id[i])
    name = SHAPES[sid].name if sid >= 0 else "probe"
    return (f"frame {i}: shape_id {sid} ({name}) len {int(wl.desc[i] & np.uint64(0xFFFF))} "
            f"parent_len {int(parent_len[i])}")

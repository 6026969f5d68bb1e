"""Chosen batches for the control-write calls (upe_gpu_ctrl_writes, upe_ctrl_writes_host,
upe_amd/ctrl.py), built from synth._frame / _eth / _arp / _ip6.  No GPU and no library needed.

chosen()        one frame per line of the issue's list — ARP, NS / NA at every frame length around
                the option, option choice, the uint8_t opt_len wrap — each with what
                handle_control_packet (reference src/worker.c:23-104) does with it, written by
                hand: NOT_MARKED, NO_RECORD (marked, nothing learned) or (kind, mac_off, mac, ip).
pack()          frames -> a batch; poison=True fills the bytes from each frame's len to the next
                frame with two well-formed options (one per kind) and 0xFF, where the clean copy
                has zeros.  The records of both copies must be identical.
placement()     n packets of plain traffic with writing packets placed by a pattern, at the sizes
                around a wave and a workgroup (UPE_CTRL_BLOCK).
with_control()  tests/test_gpu_control.with_control, copied: the stream the segmented GPU test uses.
"""
from __future__ import annotations

import numpy as np

from upe_amd import synth
from upe_amd.layout import CW_ARP, CW_NDP, desc_lens, desc_offsets, make_desc

BLOCK = 1024   # UPE_CTRL_BLOCK
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 1)
PATTERNS = ("none", "all", "first", "last", "edges", "mix")
NOT_MARKED, NO_RECORD = "not marked", "no record"

MAC_A = bytes.fromhex("0a1b2c3d4e5f")
MAC_B = bytes.fromhex("0b0102030405")
MAC_P = bytes.fromhex("0c0c0c0c0c0c")          # only ever in the poison
V6_SRC = bytes.fromhex("20010db80000000000000000000000a1")
V6_DST = bytes.fromhex("20010db80000000000000000000000b2")
V6_TGT = bytes.fromhex("fe8000000000000002112233445566c3")
SPA = 0xC0A80A07


def arp(op=1, sha=MAC_A, spa=SPA, tpa=0x0A800001, **kw) -> bytes:
    return synth._frame(synth._eth(0x0806, dst=b"\xff" * 6), synth._arp(op, sha, spa, bytes(6), tpa, **kw))


def nd(kind: int, opts: bytes = b"", nh: int = 58) -> bytes:
    """An NS (kind 135) or NA (136) of 78 bytes plus its options."""
    return synth._frame(synth._eth(0x86DD), synth._ip6(nh, V6_SRC, V6_DST, plen=24 + len(opts)),
                        bytes([kind, 0, 0, 0, 0, 0, 0, 0]) + V6_TGT, opts)


def opt(t: int, mac: bytes = MAC_A, length: int = 1) -> bytes:
    """An option of type t whose length byte is `length`, 8 bytes unless length says more."""
    body = bytes([t, length]) + mac
    size = (length * 8) & 0xFF
    return body + bytes(max(size, 8) - 8)


def _arp_rec(f: bytes, ln: int):
    at = lambda j: f[j] if j < ln else 0   # noqa: E731
    ip = bytes([at(31), at(30), at(29), at(28)]) + bytes(12)
    return (CW_ARP, 22, bytes(at(22 + j) for j in range(6)), ip)


def _nd_rec(f: bytes, off: int):
    return (CW_NDP, off + 2, f[off + 2:off + 8], f[22:38] if f[54] == 135 else f[62:78])


def _filled(kind: int, total: int) -> tuple[bytes, int]:
    """An NS / NA of `total` bytes whose matching option is the last one: fillers of several
    sizes before it, then the bytes left over (fewer than 8, zero).  Returns it and the option's
    offset."""
    want = 1 if kind == 135 else 2
    room = (total - 78) // 8 * 8 - 8
    opts = opt(5, MAC_B, 31) if room >= 248 else b""       # one 248-byte filler
    for _ in range(2):                                      # two 24-byte ones of the other kind
        if room - len(opts) >= 24:
            opts += opt(3 - want, MAC_B, 3)
    opts += opt(5, MAC_B) * ((room - len(opts)) // 8)       # 8-byte ones up to the option
    assert len(opts) == room
    f = nd(kind, opts + opt(want, MAC_A))
    return f + bytes(total - len(f)), 78 + room


def chosen():
    """[(label, frame bytes, len, expectation)]"""
    out = []

    def add(label, f, ln=None, want=NOT_MARKED):
        out.append((label, f, len(f) if ln is None else ln, want))

    # ---- ARP -------------------------------------------------------------------------------
    for op, name in ((1, "request"), (2, "reply")):
        f = arp(op)
        add(f"arp {name}", f, want=_arp_rec(f, len(f)))
    f = arp(1, tpa=synth.PORT_IP4) + bytes(18)
    add("arp request for the port address, padded to 60", f, want=_arp_rec(f, 60))
    for j in range(14, 20):
        f = bytearray(arp(1))
        f[j] ^= 0x10
        add(f"arp header byte {j} wrong", bytes(f))
    f = arp(1, sha=bytes.fromhex("f1f2f3f4f5f6"), spa=0xE1E2E3E4)
    for ln in range(14, 43):
        # the header test reads zeros past len too: 14..19 must all be there
        add(f"arp len {ln}", f, ln, _arp_rec(f, ln) if ln >= 20 else NOT_MARKED)
    # ---- NS / NA: frame lengths ------------------------------------------------------------
    for kind, name, t in ((135, "ns", 1), (136, "na", 2)):
        f = nd(kind, opt(t))
        add(f"{name} len 77", f, 77)
        for ln in range(78, 86):
            add(f"{name} len {ln}", f, ln, NO_RECORD)   # the header is readable, off + 8 > len
        add(f"{name} len 86", f, 86, _nd_rec(f, 78))
        for total in (400, 2048):
            g, off = _filled(kind, total)
            add(f"{name} len {total}, the option last", g, want=_nd_rec(g, off))
        # ---- option choice -----------------------------------------------------------------
        add(f"{name} without options", nd(kind), want=NO_RECORD)
        add(f"{name} with the other kind's option", nd(kind, opt(3 - t)), want=NO_RECORD)
        g = nd(kind, opt(5) + opt(3 - t, MAC_B) + opt(14, MAC_B, 2) + opt(t) + opt(t, MAC_B))
        add(f"{name} option after three others", g, want=_nd_rec(g, 78 + 8 + 8 + 16))
        for lb in (0, 32, 64):   # opt_len 0: the walk stops
            add(f"{name} length byte {lb} before an option",
                nd(kind, bytes([5, lb]) + bytes(6) + opt(t)), want=NO_RECORD)
        # 33 wraps to 8: the option 8 bytes on is read, never the one 264 bytes on
        g = nd(kind, bytes([5, 33]) + bytes(6) + opt(t, MAC_A) + bytes(248) + opt(t, MAC_B))
        add(f"{name} length byte 33 before an option", g, want=_nd_rec(g, 86))
        g = nd(kind, opt(t, length=33) + bytes(300))
        add(f"{name} the option's own length byte 33", g, want=_nd_rec(g, 78))
        add(f"{name} the option's own length byte 32", nd(kind, opt(t, length=32) + bytes(300)),
            want=NO_RECORD)
        add(f"{name} option longer than the frame", nd(kind, opt(t, length=2)[:8]), want=NO_RECORD)
        add(f"{name} byte 20 not 58", nd(kind, opt(t), nh=17))
    for kind in (134, 137):
        add(f"byte 54 = {kind}", nd(kind, opt(1) + opt(2)))
    add("udp", synth._frame(synth._eth(0x0800), synth._ip4(17, 0x0A000001, 0x0A800005),
                            synth._udp(1000, 53)))
    add("len 0", bytes(16), 0)
    return out


def pack(items, poison=False):
    """(frames, desc) of [(frame bytes, len)]: frame k at a 16-byte boundary with at least 16
    bytes between its len and the next frame, the bytes past len zero — or, poisoned, two
    well-formed options and 0xFF up to the next frame; UPE_FRAME_TAIL such bytes at the end."""
    lens = np.array([ln for _, ln in items], np.int64)
    slots = (lens + 16 + 15) & ~np.int64(15)
    offs = np.cumsum(slots) - slots
    total = int(slots.sum()) + 96
    frames = np.full(total, 0xFF if poison else 0, np.uint8)
    trap = np.frombuffer(opt(1, MAC_P) + opt(2, MAC_P), np.uint8)
    for (f, ln), o in zip(items, offs):
        o = int(o)
        frames[o:o + ln] = np.frombuffer(f[:ln], np.uint8)
        if poison:
            frames[o + ln:o + ln + 16] = trap
    return frames, make_desc(offs, lens)


def chosen_batch(poison=False):
    return pack([(f, ln) for _, f, ln, _ in chosen()], poison)


# ---- placement ---------------------------------------------------------------------------------

_PLAIN = synth._frame(synth._eth(0x0800), synth._ip4(17, 0x0A000001, 0x0A800005),
                      synth._udp(1000, 53)) + bytes(22)


def _writer(i: int) -> bytes:
    """A writing packet that names its position: ARP, NS and NA in turn."""
    mac = bytes([0x0A, 0x77]) + i.to_bytes(4, "big")
    if i % 3 == 0:
        return arp(1 + i % 2, sha=mac, spa=0x0A000000 + i)
    kind, t = ((135, 1), (136, 2))[i % 3 - 1]
    return nd(kind, opt(5, MAC_B) * (i % 4) + opt(t, mac))


def placement_mask(n: int, pattern: str) -> np.ndarray:
    m = np.zeros(n, bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "edges":   # the last packet of each block and the first of the next
        for b in range(BLOCK, n, BLOCK):
            m[b - 1] = m[b] = True
    elif pattern == "mix":
        m = np.random.default_rng(1000 + n).random(n) < 0.03
    else:
        assert pattern == "none"
    return m


def placement(n: int, pattern: str):
    """(frames, desc, the writing packets' positions)"""
    m = placement_mask(n, pattern)
    items = [_writer(i) if m[i] else _PLAIN for i in range(n)]
    frames, desc = pack([(f, len(f)) for f in items])
    return frames, desc, np.nonzero(m)[0]


def top_six():
    """Six control frames for a batch of 6: both kinds, a truncated ARP, a long walk, an NA that
    teaches nothing."""
    want = ("arp request", "arp len 27", "ns len 86", "na len 400, the option last",
            "na without options", "ns length byte 33 before an option")
    by = {label: (f, ln) for label, f, ln, _ in chosen()}
    return [by[k] for k in want]


# ---- the stream of tests/test_gpu_control.py ---------------------------------------------------

def _rows(wl):
    """First 128 bytes of every frame (zero past len) and the lengths."""
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    h = np.zeros((wl.n, 128), np.uint8)
    for i in range(wl.n):
        k = int(min(lens[i], 128))
        h[i, :k] = wl.frames[offs[i]:offs[i] + k]
    return h, lens.astype(np.int64)


def with_control(wl, k, seed):
    """wl with k control packets inserted at random positions (tests/test_gpu_control.py's
    generator, statement for statement: the same seed gives the same stream).  ARP packets teach
    the MACs of IPv4 destinations that later packets go to, some ask for the port address; NS / NA
    teach IPv6 destinations; a few carry no usable address (wrong hlen, no option)."""
    rng = np.random.default_rng(seed)
    h, lens = _rows(wl)
    et = (h[:, 12].astype(np.int64) << 8) | h[:, 13]
    v4 = np.nonzero(et == 0x0800)[0]
    v6 = np.nonzero(et == 0x86DD)[0]
    ctrl = []
    for j in range(k):
        mac = bytes(rng.integers(0, 256, 6, dtype=np.uint8))
        kind = rng.integers(0, 6)
        if kind <= 1 and len(v4):
            dst = int.from_bytes(bytes(h[rng.choice(v4), 30:34]), "big")
            tpa = synth.PORT_IP4 if kind == 1 else 0x0A800001
            f = synth._frame(synth._eth(0x0806, dst=b"\xff" * 6),
                             synth._arp(1, mac, dst, bytes(6), tpa))
        elif kind == 2 and len(v4):
            dst = int.from_bytes(bytes(h[rng.choice(v4), 30:34]), "big")
            f = synth._frame(synth._eth(0x0806), synth._arp(1, mac, dst, bytes(6), 0, hlen=8))
        elif kind == 3 and len(v6):
            dst = bytes(h[rng.choice(v6), 38:54])
            f = synth._frame(synth._eth(0x86DD), synth._ip6(58, dst, bytes(16)),
                             bytes([135, 0, 0, 0, 0, 0, 0, 0]) + bytes(16), bytes([1, 1]) + mac)
        elif kind == 4 and len(v6):
            dst = bytes(h[rng.choice(v6), 38:54])
            f = synth._frame(synth._eth(0x86DD), synth._ip6(58, bytes(16), dst),
                             bytes([136, 0, 0, 0, 0x60, 0, 0, 0]) + dst,
                             bytes([5, 1]) + bytes(6) + bytes([2, 1]) + mac)
        else:
            f = synth._frame(synth._eth(0x86DD), synth._ip6(58, bytes(16), bytes(16)),
                             bytes([135, 0, 0, 0, 0, 0, 0, 0]) + bytes(16))
        ctrl.append(f)
    pos = np.sort(rng.integers(0, wl.n + 1, k))
    rows, lns = [], []
    src = 0
    for p, f in zip(pos, ctrl):
        rows.append(h[src:p])
        lns.append(lens[src:p])
        r = np.zeros((1, 128), np.uint8)
        r[0, :len(f)] = np.frombuffer(f, np.uint8)
        rows.append(r)
        lns.append(np.array([len(f)], np.int64))
        src = p
    rows.append(h[src:])
    lns.append(lens[src:])
    frames, desc = synth.pack_frames(np.concatenate(rows), np.concatenate(lns))
    return synth.Workload(wl.name + "+ctrl", frames, desc, wl.rules, wl.capacity, wl.arp.copy(),
                          wl.ndp.copy(), wl.eth_addr, wl.ip4_addr, wl.l1.copy())

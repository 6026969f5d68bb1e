"""Batches whose forwarded set is chosen, and the emit-mode outputs they must give.

Emit mode (include/upe_gpu.h) writes a 16-byte record for forwarded packets only, at
64 * (i / 64) + the packet's rank among the forwarded packets of its 64-packet group (a ballot and
a lane count in upe_classify); upe_gpu_process_emit_tx adds tx[] and tx_count[] by the same
arithmetic, repair_deferred rewrites records through the slot it saved, and upe_gpu_compact
builds the flat list.  The synthetic workloads forward whatever their traffic model gives: a group
that forwards nothing, everything, only lane 0, only lane 63 or only lanes 31 and 32 (the seam
between the two halves of the lane count) never occurs in them.  Here the kind of every packet is
chosen (build), so the forwarded set is known before anything runs; the groups follow named lane
patterns (patterns), put next to each other in every order (sequences), and the expected outputs
(expected) come from the C restatement of the reference worker alone, laid out over a poison that
no record can equal, so that a slot the kernel must not write is seen when it is written.

Rule table (table): four probe rules among exact (source port, destination port) filler rules that
no packet carries, as accounting_cases.table builds them.  The probes: forward UDP over IPv4 by one
destination port (the first sorted index), drop by a second port and an action that is neither
DROP nor FWD by a third (two neighbouring middle indexes; synth.make_rule and the restatement
both represent it: UPE_V_DROP_ACTION), forward IPv6 by the first port (the last sorted index).
Sizes: 8 (the small-table kernel), 1000 (family lists, tree or scan, as forced) and
ac.LDS_LAST + 1, past the LDS rule_stats bins: with so few mask signatures that one is matched
through the tuple space unless a scan or the tree is forced, and either way the launch writes the
group-by's side array.

Neighbours (neighbours): 16 destinations of each family have an entry, 16 have none.  big=False:
slot arrays of 1024, whose index the kernels stage in LDS (the lean kernels).  big=True: slot
arrays of 8192 that also hold BIG_FILL entries no packet is sent to: the device index is sized by
the reachable entries, not by the slot array (neigh_cases.FILLERS), and only past 1638 of them does
it outgrow the staged size, which is what selects the kernels that are not lean.

tests/test_egress_cases.py pins all of this on the CPU; tests/test_gpu_egress_cases.py then runs
the batches through every emit launch form.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import accounting_cases as ac
import oracle
from test_emit_records import records_from_reference
from upe_amd import gpu, synth
from upe_amd.layout import (ACT_DROP, ACT_FWD, RULE_DTYPE, V_CONSUMED, V_DROP_ACTION,
                            V_DROP_NOMATCH, V_DROP_PARSE, V_DROP_RULE, V_DROP_TTL, V_FWD,
                            VF_ARP_LEARN, VF_ARP_REPLY, VF_NEIGH_HIT, desc_lens, desc_offsets)

# ---------------------------------------------------------------------------------------------
# kinds
# ---------------------------------------------------------------------------------------------

(FWD4_HIT, FWD4_MISS, FWD6_HIT, FWD6_MISS, DROP_RULE, NOMATCH, DROP_ACTION, TTL1, SHORT, CONSUMED,
 ARP_REPLY) = range(11)
KIND_NAMES = ("FWD4_HIT", "FWD4_MISS", "FWD6_HIT", "FWD6_MISS", "DROP_RULE", "NOMATCH",
              "DROP_ACTION", "TTL1", "SHORT", "CONSUMED", "ARP_REPLY")
FWD_KINDS = (FWD4_HIT, FWD4_MISS, FWD6_HIT, FWD6_MISS)
OTHER_KINDS = (DROP_RULE, NOMATCH, DROP_ACTION, TTL1, SHORT, CONSUMED, ARP_REPLY)
# kinds whose frame is the same 64-byte UDP over IPv4 frame but for addresses and ports: a packet
# can change between them without its descriptor changing (three_passes)
SAME_FRAME = (FWD4_HIT, FWD4_MISS, DROP_RULE, NOMATCH, DROP_ACTION)
# the verdict word each kind must get, without its rule bits
KIND_VERDICT = np.array([V_FWD | VF_NEIGH_HIT, V_FWD, V_FWD | VF_NEIGH_HIT, V_FWD, V_DROP_RULE,
                         V_DROP_NOMATCH, V_DROP_ACTION, V_DROP_TTL, V_DROP_PARSE, V_CONSUMED,
                         V_DROP_PARSE | VF_ARP_LEARN | VF_ARP_REPLY], np.uint32)
NO_RULE_BITS = np.uint32(0xFF)

PORT_FWD, PORT_DROP, PORT_ACTION, PORT_NONE = 40000, 40001, 40002, 40003
SPORT = 50000                      # filler rules' source ports stay far below (ac.table)
NEIGH = 16                         # destinations with an entry, and without, per family
HIT4 = 0x0A800010 + np.arange(NEIGH, dtype=np.uint64)       # 10.128.0.16 ...
MISS4 = 0x0A800110 + np.arange(NEIGH, dtype=np.uint64)      # 10.128.1.16 ...
SRC4 = 0x0A000001
BIG_FILL = 1700                    # 5 * (1700 + 16) > 4 * 2048: the index takes 4096 slots
TABLE_SIZES = (8, 1000, ac.LDS_LAST + 1)
POISON = 0xA5                      # b[15] of a record is 4 or 6, of a zero record 0
POISON32 = np.uint32(0xA5A5A5A5)   # no packet index, and no count, comes near it
CANARY = 64                        # records, entries and counts behind every output


def _v6(group: int, j: int) -> bytes:
    return bytes.fromhex("2001db80") + bytes(8) + bytes([0, group, 1, j])


HIT6 = np.array([np.frombuffer(_v6(0, j), np.uint8) for j in range(NEIGH)])
MISS6 = np.array([np.frombuffer(_v6(1, j), np.uint8) for j in range(NEIGH)])
SRC6 = np.frombuffer(bytes.fromhex("20010db8") + bytes(11) + b"\x01", np.uint8)


def neigh_mac(fam: int, j: int) -> bytes:
    return bytes([0x02, 0xE0 | fam, 0x11, 0x22, 0x33, j])


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Table:
    nrules: int
    rules: np.ndarray          # insertion order
    rules_sorted: np.ndarray
    capacity: int
    probe_index: dict          # sorted index of each probe rule


_TABLES: dict = {}
_NEIGH: dict = {}


def table(nrules: int) -> Table:
    if nrules not in _TABLES:
        assert nrules >= 8
        mid = nrules // 2
        probe_index = {"fwd4": 0, "drop": mid - 1, "action": mid, "fwd6": nrules - 1}
        probes = [synth.make_rule(0, ACT_FWD, ip_ver=4, proto=17, dport=PORT_FWD),
                  synth.make_rule(mid - 1, ACT_DROP, dport=PORT_DROP),
                  synth.make_rule(mid, 2, dport=PORT_ACTION),
                  synth.make_rule(nrules - 1, ACT_FWD, ip_ver=6, dport=PORT_FWD)]
        k = np.arange(nrules - 4)
        f = np.zeros(nrules - 4, RULE_DTYPE)
        free = np.setdiff1d(np.arange(nrules), list(probe_index.values()))
        f["priority"] = free[np.random.default_rng([17, nrules]).permutation(len(free))]
        f["ip_ver"] = 4
        f["protocol"] = 17
        f["dst_port"] = 1 + k % ac.PORT_SPAN
        f["src_port"] = 1 + k // ac.PORT_SPAN
        f["action"] = np.where(k % 2 == 1, ACT_DROP, ACT_FWD)
        f["out_ifindex"] = np.where(k % 2 == 1, 0, 1)
        rules = np.concatenate([f[:len(f) // 2], synth.rules_array(probes), f[len(f) // 2:]])
        rs = synth.build_rule_table(rules)
        cap = 1024
        while cap < nrules:
            cap *= 2
        assert rs["priority"].tolist() == list(range(nrules))
        t = Table(nrules, rules, rs, cap, probe_index)
        for a in (t.rules, t.rules_sorted):
            a.setflags(write=False)
        _TABLES[nrules] = t
    return _TABLES[nrules]


def neighbours(big: bool):
    """(arp, ndp) slot arrays: the NEIGH hit destinations of each family, in 1024 slots, or in
    8192 slots beside BIG_FILL entries of other addresses."""
    if big not in _NEIGH:
        rng = np.random.default_rng(23)
        cap = 8192 if big else 1024
        e4 = [(int(HIT4[j]), neigh_mac(4, j)) for j in range(NEIGH)]
        e6 = [(HIT6[j].tobytes(), neigh_mac(6, j)) for j in range(NEIGH)]
        if big:
            for x in rng.choice(1 << 20, size=BIG_FILL, replace=False):
                e4.append((0x0AC00000 + int(x), synth._rand_macs(rng, 1)[0].tobytes()))
                e6.append((bytes.fromhex("2001db81") + bytes(8) + int(x).to_bytes(4, "big"),
                           synth._rand_macs(rng, 1)[0].tobytes()))
        arp, ndp = synth.arp_table(cap, e4), synth.ndp_table(cap, e6)
        assert int(arp["valid"].sum()) == len(e4) and int(ndp["valid"].sum()) == len(e6)
        arp.setflags(write=False)
        ndp.setflags(write=False)
        _NEIGH[big] = (arp, ndp)
    return _NEIGH[big]


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Batch:
    name: str
    kinds: np.ndarray
    frames: np.ndarray
    desc: np.ndarray

    @property
    def n(self) -> int:
        return len(self.kinds)

    @property
    def fwd(self) -> np.ndarray:
        return np.isin(self.kinds, FWD_KINDS)


def build(kind_per_packet, name: str = "", one_dst4: bool = False, other_at: int = -1) -> Batch:
    """Frames and descriptors for packets of the given kinds.  Packet i carries i in its source
    MAC (bytes 7..10 of the frame) and in its IPv4 id, and the TTL or hop limit 2 + i % 250, so
    that no two forwarded packets fewer than 250 apart share a record; its destination is entry
    (7 i + i / 64) % NEIGH of the hit or the miss addresses.  one_dst4: every FWD4_HIT packet goes
    to HIT4[0] (the look-back test aims them at one L1 entry), except packet other_at, which goes
    to HIT4[1]: it misses the entry and hits the table, after which the entry is no longer used."""
    kinds = np.asarray(kind_per_packet, np.int64)
    n = len(kinds)
    i = np.arange(n)
    odd = i % 2 == 1
    v6 = np.isin(kinds, (FWD6_HIT, FWD6_MISS, CONSUMED)) | ((kinds == TTL1) & odd)
    arp = kinds == ARP_REPLY
    v4 = ~v6 & ~arp
    h = np.zeros((n, 96), np.uint8)
    h[:, 0:6] = (0x02, 0x10, 0x20, 0x30, 0x40, 0x50)
    h[:, 6] = 0x02
    for k in range(4):
        h[:, 7 + k] = (i >> (24 - 8 * k)) & 0xFF
    h[:, 11] = 0x5A
    j = (7 * i + i // 64) % NEIGH
    ttl = np.where(kinds == TTL1, 1, 2 + i % 250)
    dport = np.select([kinds == DROP_RULE, kinds == DROP_ACTION, kinds == NOMATCH],
                      [PORT_DROP, PORT_ACTION, PORT_NONE], PORT_FWD).astype(np.uint32)
    sport = np.full(n, SPORT, np.uint32)
    lens = np.full(n, 64, np.int64)

    r4 = np.nonzero(v4)[0]
    hit4 = np.isin(kinds[r4], (FWD4_HIT, TTL1))
    j4 = np.where(one_dst4 & (kinds[r4] == FWD4_HIT), np.where(r4 == other_at, 1, 0), j[r4])
    synth.build_ipv4(h, r4, src=np.full(len(r4), SRC4, np.uint64),
                     dst=np.where(hit4, HIT4[j4], MISS4[j4]), proto=np.full(len(r4), 17),
                     ttl=ttl[r4], ihl=np.full(len(r4), 5), total_len=np.full(len(r4), 50),
                     l4_ports=(sport[r4], dport[r4]))
    h[r4, 18] = (r4 >> 8) & 0xFF                   # the IPv4 id, then the checksum again
    h[r4, 19] = r4 & 0xFF
    cs = synth.ipv4_header_checksum(h[r4], np.full(len(r4), 5, np.int64))
    h[r4, 24], h[r4, 25] = cs >> 8, cs & 0xFF
    h[r4, 39] = 30                                 # the UDP length
    lens[kinds == SHORT] = 20                      # cut inside the IPv4 header

    r6 = np.nonzero(v6)[0]
    hit6 = np.isin(kinds[r6], (FWD6_HIT, TTL1))
    ns = kinds[r6] == CONSUMED
    synth.build_ipv6(h, r6, src16=np.tile(SRC6, (len(r6), 1)),
                     dst16=np.where(hit6[:, None], HIT6[j[r6]], MISS6[j[r6]]),
                     nh=np.where(ns, 58, 17), hop=ttl[r6],
                     payload_len=np.where(ns, 24, 16), sport=sport[r6], dport=dport[r6])
    rn = r6[ns]                                    # a neighbour solicitation without an option
    h[rn, 54:78] = 0
    h[rn, 54] = 135
    h[rn, 62:78] = HIT6[j[rn]]
    lens[r6] = np.where(ns, 78, 70)

    for r in np.nonzero(arp)[0]:                   # an ARP request for the port's address
        fr = synth._frame(synth._eth(0x0806, dst=b"\xff" * 6, src=h[r, 6:12].tobytes()),
                          synth._arp(1, h[r, 6:12].tobytes(), 0x0A800200 + int(r) % 251, bytes(6),
                                     synth.PORT_IP4))
        h[r] = 0
        h[r, :len(fr)] = np.frombuffer(fr, np.uint8)
    lens[arp] = 60
    frames, desc = synth.pack_frames(h, lens)
    return Batch(name or f"kinds:{n}", kinds, frames, desc)


def workload(b: Batch, t: Table, big: bool = False) -> synth.Workload:
    arp, ndp = neighbours(big)
    return synth.Workload(b.name, b.frames, b.desc, t.rules, t.capacity, arp, ndp)


# ---------------------------------------------------------------------------------------------
# lane patterns, and the kinds of a batch that follows them
# ---------------------------------------------------------------------------------------------

def patterns() -> dict:
    """name -> 64 booleans: the lanes of a group that forward."""
    lane = np.arange(64)
    rng = np.random.default_rng(29)
    p = {"empty": lane < 0, "full": lane >= 0, "lane0": lane == 0, "lane63": lane == 63,
         "seam": (lane == 31) | (lane == 32), "low": lane < 32, "high": lane >= 32,
         "even": lane % 2 == 0, "odd": lane % 2 == 1,
         "eighth": rng.random(64) < 1 / 8, "seven_eighths": rng.random(64) < 7 / 8}
    assert 0 < p["eighth"].sum() < 32 < p["seven_eighths"].sum() < 64
    return p


def kinds_of(fwd_mask: np.ndarray) -> np.ndarray:
    """Kinds for a batch with the given forwarded set: the forwarding lanes cycle through the four
    forwarded kinds, the others through every kind that does not forward."""
    m = np.asarray(fwd_mask, bool)
    rank_f = np.cumsum(m) - 1
    rank_o = np.cumsum(~m) - 1
    return np.where(m, np.asarray(FWD_KINDS)[rank_f % len(FWD_KINDS)],
                    np.asarray(OTHER_KINDS)[rank_o % len(OTHER_KINDS)])


def euler_circuit(k: int) -> list:
    """0..k-1 in an order (k * k + 1 long) in which every ordered pair, a value with itself
    included, occurs as neighbours: an Euler circuit of the complete directed graph (Hierholzer)."""
    nxt = [0] * k
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append((v + 1 + nxt[v]) % k)   # the loop v -> v last
            nxt[v] += 1
        else:
            out.append(stack.pop())
    out.reverse()
    assert set(zip(out[:-1], out[1:])) == {(a, b) for a in range(k) for b in range(k)}
    assert len(out) == k * k + 1
    return out


def pair_order() -> list:
    """The pattern names in such an order."""
    names = list(patterns())
    return [names[v] for v in euler_circuit(len(names))]


def pair_mask() -> np.ndarray:
    p = patterns()
    return np.concatenate([p[name] for name in pair_order()])


SMALL_CUTS = (1, 31, 63, 64, 65)
TAIL_EXTRA = (1, 31, 33, 63)


def tail_cut(mask: np.ndarray, n: int, forwards: bool) -> np.ndarray:
    """The forwarded set cut to n packets, its last group (whole or ragged) forwarding only its
    last live lane, or nothing."""
    m = mask[:n].copy()
    m[(n - 1) // 64 * 64:] = False
    m[n - 1] = forwards
    return m


_SEQ: dict = {}


def sequences() -> dict:
    """name -> Batch."""
    if not _SEQ:
        mask = pair_mask()
        whole = len(mask) - 64
        _SEQ["pairs"] = build(kinds_of(mask), "pairs")
        for n in SMALL_CUTS + tuple(whole + r for r in TAIL_EXTRA):
            for forwards in (True, False):
                name = f"cut:{n}:{'last' if forwards else 'none'}"
                _SEQ[name] = build(kinds_of(tail_cut(mask, n, forwards)), name)
        _SEQ["all_empty"] = build(kinds_of(np.zeros(5 * 64 + 17, bool)), "all_empty")
        _SEQ["all_full"] = build(kinds_of(np.ones(5 * 64 + 17, bool)), "all_full")
    return _SEQ


def tiled(n: int) -> Batch:
    """The pair sequence repeated up to n packets."""
    return build(np.resize(kinds_of(pair_mask()), n), f"tiled:{n}")


def three_passes() -> list:
    """Three batches over one descriptor array whose forwarded sets differ: the pair sequence,
    and twice the same with every packet of a SAME_FRAME kind moved on to another of them."""
    k0 = kinds_of(pair_mask())
    same = np.isin(k0, SAME_FRAME)
    pos = np.searchsorted(np.asarray(SAME_FRAME), np.where(same, k0, SAME_FRAME[0]))
    out = [build(k0, "pass0")]
    for p in (1, 2):
        step = p * (1 + np.arange(len(k0)) % 2)
        kp = np.where(same, np.asarray(SAME_FRAME)[(pos + step) % len(SAME_FRAME)], k0)
        out.append(build(kp, f"pass{p}"))
        assert np.array_equal(out[-1].desc, out[0].desc)
        assert (out[-1].fwd != out[0].fwd).sum() > len(k0) // 8
    return out


# ---------------------------------------------------------------------------------------------
# expected outputs
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Expected:
    n: int
    verdict: np.ndarray     # n
    records: np.ndarray     # (n, 16), zero for a packet not forwarded
    slots: np.ndarray       # per packet (meaningful for forwarded ones)
    raw: np.ndarray         # (n + CANARY, 16): poison, the records at their slots
    tx: np.ndarray          # n + CANARY: poison, the packet indexes at their slots
    tx_count: np.ndarray    # groups + CANARY: every group's count, then poison
    fwd_list: np.ndarray    # the flat list
    frames: np.ndarray      # what emit mode leaves: the input but for answered ARP requests
    frames_applied: np.ndarray   # the restatement's frames (records applied)
    counters: np.ndarray
    rule_stats: np.ndarray
    l1: np.ndarray

    @property
    def groups(self) -> int:
        return (self.n + 63) // 64


def layout(verdict: np.ndarray, records: np.ndarray, base: int = 0, total: int | None = None):
    """(raw, tx, tx_count, slots) of one launch over packets base .. base + len(verdict) - 1 of a
    buffer of `total` packets (default: the launch's own), canary behind: records and tx entries
    are counted from the launch's first packet, tx holds indexes relative to it."""
    n = len(verdict)
    total = n if total is None else total
    raw = np.full((total + CANARY, 16), POISON, np.uint8)
    tx = np.full(total + CANARY, POISON32, np.uint32)
    cnt = np.full((total + 63) // 64 + CANARY, POISON32, np.uint32)
    fwd = (verdict & 0xF) == V_FWD
    slots = gpu.record_slots(verdict)
    raw[base + slots[fwd]] = records[fwd]
    tx[base + slots[fwd]] = np.nonzero(fwd)[0]
    if base == 0:
        cnt[:(n + 63) // 64] = np.bincount(np.nonzero(fwd)[0] // 64, minlength=(n + 63) // 64)
    return raw, tx, cnt, slots


def assert_unique(records: np.ndarray, span: int = 128) -> None:
    """Any two forwarded packets fewer than `span` positions apart have different records (so a
    record in a neighbouring slot, or in the slot of the next group, is seen)."""
    w = np.ascontiguousarray(records).view("<u8").reshape(-1, 2)
    fwd = records[:, 15] != 0
    for d in range(1, min(span, len(w))):
        same = fwd[d:] & fwd[:-d] & (w[d:] == w[:-d]).all(axis=1)
        assert not same.any(), f"packets {_first_bad(same)} and {_first_bad(same) + d} share a record"


def expected(wl: synth.Workload, **state) -> Expected:
    """Everything an emit launch over the workload must leave, from the restatement alone.
    state: l1, counters, rule_stats to start from (a launch after others)."""
    r = oracle.run_restated(wl, apply_control=False, **state)
    rec = records_from_reference(wl.frames, r.frames, wl.desc, r.verdict)
    assert_unique(rec)
    raw, tx, cnt, slots = layout(r.verdict, rec)
    frames = wl.frames.copy()
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    for i in np.nonzero(r.verdict & VF_ARP_REPLY)[0]:
        o, ln = int(offs[i]), min(int(lens[i]), 48)
        frames[o:o + ln] = r.frames[o:o + ln]
    return Expected(wl.n, r.verdict, rec, slots, raw, tx, cnt,
                    np.nonzero((r.verdict & 0xF) == V_FWD)[0], frames, r.frames, r.counters,
                    r.rule_stats, r.l1)


def expected_chain(wl: synth.Workload, cuts) -> list:
    """expected() of each piece cuts[k] .. cuts[k + 1] of the batch run as a launch of its own
    after the pieces before it (the worker's state carried over)."""
    out, state = [], {}
    for s, e in zip(cuts[:-1], cuts[1:]):
        piece = dataclasses.replace(wl, desc=wl.desc[s:e])
        out.append(expected(piece, **state))
        state = {"l1": out[-1].l1, "counters": out[-1].counters,
                 "rule_stats": out[-1].rule_stats}
    return out


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------

def _first_bad(bad: np.ndarray) -> int:
    return int(np.nonzero(bad)[0][0])


def check_layout(exp_raw=None, raw=None, exp_tx=None, tx=None, exp_count=None, tx_count=None,
                 what: str = "", only=None) -> None:
    """The raw record array, the egress list and its counts against the expected ones, bit for
    bit, canary included; a difference is reported with its 64-packet group and its slot.
    only: a boolean per record slot, the slots to compare (default: all)."""
    if raw is not None:
        got = np.ascontiguousarray(raw, np.uint8).reshape(-1, 16)
        assert got.shape == exp_raw.shape, f"{what}: {got.shape[0]} record slots"
        bad = (got != exp_raw).any(axis=1)
        if only is not None:
            bad &= only
        if bad.any():
            s = _first_bad(bad)
            want = ("no record (poison)" if (exp_raw[s] == POISON).all()
                    else exp_raw[s].tobytes().hex())
            have = ("untouched (poison)" if (got[s] == POISON).all() else got[s].tobytes().hex())
            raise AssertionError(f"{what}: records differ in {int(bad.sum())} slots, first in "
                                 f"group {s // 64} slot {s} (lane {s % 64}): want {want}, "
                                 f"got {have}")
    if tx_count is not None:
        got = np.asarray(tx_count, np.uint32)
        assert got.shape == exp_count.shape, f"{what}: {got.shape[0]} counts"
        bad = got != exp_count
        if bad.any():
            g = _first_bad(bad)
            raise AssertionError(f"{what}: tx_count differs for {int(bad.sum())} groups, first "
                                 f"group {g} (slot {64 * g}): want {int(exp_count[g]):#x}, got "
                                 f"{int(got[g]):#x}")
    if tx is not None:
        got = np.asarray(tx, np.uint32)
        assert got.shape == exp_tx.shape, f"{what}: {got.shape[0]} tx entries"
        bad = got != exp_tx
        if bad.any():
            s = _first_bad(bad)
            raise AssertionError(f"{what}: tx differs in {int(bad.sum())} entries, first in "
                                 f"group {s // 64} slot {s} (lane {s % 64}): want "
                                 f"{int(exp_tx[s]):#x}, got {int(got[s]):#x}")


def check_expected(exp: Expected, what: str, raw=None, tx=None, tx_count=None) -> None:
    check_layout(exp.raw, raw, exp.tx, tx, exp.tx_count, tx_count, what)

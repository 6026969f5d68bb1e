"""Rule tables and batches whose rule_stats and counters are known before anything runs.

The accounting of the GPU path (upe_amd/csrc/upe_gpu.hip) takes three routes by table size: up to
kSmallRules padded rules a workgroup's LDS bins go into replicated accumulators, up to kLdsStatsMax
into replicas per sorted index, past that a group-by over the batch (upe_rule_hist,
upe_hist_reduce) in ranges of kHistRange rules and chunks of at least kHistChunkMin packets, with
4-byte keys up to 65536 rules.  The synthetic workloads hit rules as their traffic model happens
to; the tables here sit on those sizes, and every batch names the sorted index each packet matches
and its length, so the expected rule_stats and counters are a bincount (expected()).

A table of `nrules` rules: rule k matches UDP over IPv4 with one exact (source port, destination
port) pair, pairs distinct, so exactly one probe flow matches it and that flow matches no other
rule; priorities are a permutation of 0..nrules-1, so rule k's sorted index is its priority (and
differs from its rule_id, k); odd sorted indexes drop, even ones forward.  One flow matches nothing.

A packet aimed at a forwarding rule owns its frame (an in-place run rewrites it); packets aimed at
a dropping rule, or at nothing, may share one frame per (rule, length), so a long frame exists once
however many descriptors point at it, and only a dropping rule ever sees one.

tests/test_accounting_cases.py pins all of this on the CPU against the oracle;
tests/test_gpu_accounting.py then runs the batches through the kernels.
"""
from __future__ import annotations

import dataclasses
import os
import re

import numpy as np

from keyframes import RUN
from upe_amd import synth
from upe_amd.layout import (ACT_DROP, ACT_FWD, ARP_DTYPE, COUNTERS_DTYPE, NDP_DTYPE, RULE_DTYPE,
                            RULE_STAT_DTYPE, V_DROP_NOMATCH, V_DROP_RULE, V_FWD, make_desc)

# ---------------------------------------------------------------------------------------------
# the sizes the device code branches on, read from its headers
# ---------------------------------------------------------------------------------------------

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "upe_amd", "csrc")


def _const(header: str, pattern: str) -> int:
    with open(os.path.join(_CSRC, header)) as f:
        m = re.search(pattern, f.read())
    assert m, f"{header}: {pattern} not found"
    return int(m.group(1))


K_UNROLL = _const("upe_dev.h", r"constexpr int kUnroll = (\d+);")
K_SMALL_RULES = _const("upe_dev.h", r"constexpr int kSmallRules = (\d+);")
K_LDS_STATS_MAX = _const("upe_plan.h", r"#define UPE_LDS_STATS_MAX (\d+)")
K_HIST_RANGE = _const("upe_plan.h", r"#define UPE_HIST_RANGE (\d+)")
K_HIST_CHUNK_MIN = _const("upe_plan.h", r"constexpr uint32_t kHistChunkMin = (\d+);")
K_GB_PACKED = _const("upe_plan.h", r"p\.gb_packed = t\.nrules <= (\d+)u")   # rules with 4-byte keys
K_WG_PACKETS = _const("upe_plan.h", r"constexpr size_t kWgPackets = (\d+);")


def nrules_pad(nrules: int) -> int:
    """upe_rules.cpp build_image: whole blocks of kUnroll rules plus one padding block."""
    return ((nrules + K_UNROLL - 1) // K_UNROLL + 1) * K_UNROLL


def stats_path(nrules: int) -> str:
    pad = nrules_pad(nrules)
    return "small" if pad <= K_SMALL_RULES else "mid" if pad <= K_LDS_STATS_MAX else "group-by"


def _largest_with_pad(limit: int) -> int:
    n = limit
    while nrules_pad(n) > limit:
        n -= 1
    return n


SMALL_LAST = _largest_with_pad(K_SMALL_RULES)      # the last table of the small path (60 rules)
LDS_LAST = _largest_with_pad(K_LDS_STATS_MAX)      # the last table with LDS bins (4092 rules)
TABLE_SIZES = (8, SMALL_LAST, SMALL_LAST + 1, 1000, LDS_LAST, LDS_LAST + 1, K_HIST_RANGE,
               K_HIST_RANGE + 1, K_GB_PACKED, K_GB_PACKED + 1)
BATCH_SIZES = (1, 63, 64, 65, K_HIST_CHUNK_MIN - 1, K_HIST_CHUNK_MIN, K_HIST_CHUNK_MIN + 1,
               K_HIST_CHUNK_MIN + 15, 2 * K_HIST_CHUNK_MIN + 1, 40005)
LENS = (60, 1514, 65535)
MOST = 2048          # rules a batch aims at when the table has more than it has room for
LONG_RULES = 12      # dropping rules of a batch that get 65535-byte frames, boundary indexes first
NONE = -1            # a packet's target when it matches nothing

PORT_SPAN = 60000                       # destination ports 1..PORT_SPAN, then the next source port
NOMATCH_PORTS = (65000, 1)              # source ports of rules stay far below 65000
SRC_IP, DST_IP = 0x0A000001, 0x0A8000C8   # 10.0.0.1 -> 10.128.0.200 (no neighbour entry)
ARP_IP = 0x0A800007                     # the one neighbour entry, for the look-back test's L1 start


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Table:
    nrules: int
    rules: np.ndarray          # insertion order: rule k has rule_id k
    rules_sorted: np.ndarray   # synth.build_rule_table(rules)
    capacity: int
    sorted_index: np.ndarray   # of rule k (= its priority)
    rule_id: np.ndarray        # of sorted index s
    sport: np.ndarray          # of sorted index s: the probe flow's ports
    dport: np.ndarray
    drops: np.ndarray          # of sorted index s: the rule drops

    @property
    def path(self) -> str:
        return stats_path(self.nrules)

    def boundaries(self) -> dict:
        """The sorted indexes the accounting treats specially, where the table has them."""
        b = {"first": 0, "last": self.nrules - 1, "range0_last": K_HIST_RANGE - 1,
             "range1_first": K_HIST_RANGE, "key_max": K_GB_PACKED - 1, "past_key": K_GB_PACKED}
        return {k: v for k, v in b.items() if v < self.nrules}


_TABLES: dict = {}


def table(nrules: int) -> Table:
    if nrules not in _TABLES:
        rng = np.random.default_rng([11, nrules])
        k = np.arange(nrules)
        r = np.zeros(nrules, RULE_DTYPE)
        prio = rng.permutation(nrules)
        r["priority"] = prio
        r["ip_ver"] = 4
        r["protocol"] = 17
        r["dst_port"] = 1 + k % PORT_SPAN
        r["src_port"] = 1 + k // PORT_SPAN
        drops = prio % 2 == 1
        r["action"] = np.where(drops, ACT_DROP, ACT_FWD)
        r["out_ifindex"] = np.where(drops, 0, 1)
        rs = synth.build_rule_table(r)
        cap = 1024
        while cap < nrules:
            cap *= 2
        rid = np.empty(nrules, np.int64)
        rid[prio] = k
        t = Table(nrules, r, rs, cap, prio.astype(np.int64), rid,
                  rs["src_port"].astype(np.int64), rs["dst_port"].astype(np.int64),
                  rs["action"] == ACT_DROP)
        for a in (t.rules, t.rules_sorted, t.sorted_index, t.rule_id, t.sport, t.dport, t.drops):
            a.setflags(write=False)
        _TABLES[nrules] = t
    return _TABLES[nrules]


def neighbours():
    """One ARP entry (the look-back test starts from an L1 entry that contradicts it); no packet
    of these batches is sent to it, so no frame's MACs change."""
    arp = synth.arp_table(16, [(ARP_IP, bytes.fromhex("02aabbccdd07"))])
    return arp, np.zeros(0, NDP_DTYPE)


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Batch:
    name: str
    target: np.ndarray   # per packet: the sorted index it matches, or NONE
    lens: np.ndarray     # per packet: its descriptor length
    frames: np.ndarray
    desc: np.ndarray
    shared: int          # descriptors that point at a frame another descriptor points at

    @property
    def n(self) -> int:
        return len(self.target)


def rule_len(t: Table, idx: np.ndarray, long_set) -> np.ndarray:
    """The length every packet aimed at sorted index idx carries in a batch: neighbouring indexes
    differ, a forwarding rule's frames stay short (each packet owns one), every sixteenth dropping
    rule gets 1514, the dropping rules of `long_set` 65535."""
    idx = np.asarray(idx, np.int64)
    out = np.where(t.drops[idx], 61 + idx % 59, 60 + (idx // 2) % 61)
    out = np.where(t.drops[idx] & (idx % 16 == 1), LENS[1], out)
    if len(long_set):
        out = np.where(np.isin(idx, np.asarray(list(long_set))) & t.drops[idx], LENS[2], out)
    return out


def build(t: Table, name: str, target: np.ndarray, lens: np.ndarray) -> Batch:
    """Frames and descriptors for packets with the given targets and lengths."""
    target = np.asarray(target, np.int64)
    lens = np.asarray(lens, np.int64)
    n = len(target)
    hit = target >= 0
    safe = np.where(hit, target, 0)
    own = hit & ~t.drops[safe]                      # forwarded: rewritten in place
    assert (lens[own] <= 200).all(), "a long frame may only meet a dropping rule"
    # frame of packet i: its own, or the one of its (target, length)
    key = (target + 1) * 65536 + lens
    uniq, inv = np.unique(key[~own], return_inverse=True)
    frame_of = np.empty(n, np.int64)
    frame_of[own] = np.arange(int(own.sum()))
    frame_of[~own] = int(own.sum()) + inv
    nf = int(own.sum()) + len(uniq)
    ftarget = np.empty(nf, np.int64)
    flen = np.empty(nf, np.int64)
    ftarget[frame_of] = target
    flen[frame_of] = lens
    fhit = ftarget >= 0
    fsafe = np.where(fhit, ftarget, 0)
    sport = np.where(fhit, t.sport[fsafe], NOMATCH_PORTS[0]).astype(np.uint32)
    dport = np.where(fhit, t.dport[fsafe], NOMATCH_PORTS[1]).astype(np.uint32)
    h = np.zeros((nf, 64), np.uint8)
    h[:, 0:6] = (0x02, 0x10, 0x20, 0x30, 0x40, 0x50)
    h[:, 6:12] = (0x02, 0x60, 0x70, 0x80, 0x90, 0xA0)
    rows = np.arange(nf)
    synth.build_ipv4(h, rows, src=np.full(nf, SRC_IP, np.uint64), dst=np.full(nf, DST_IP, np.uint64),
                     proto=np.full(nf, 17), ttl=np.full(nf, 64), ihl=np.full(nf, 5),
                     total_len=flen - 14, l4_ports=(sport, dport))
    frames, fdesc = synth.pack_frames(h, flen)
    offs = (fdesc >> np.uint64(16)).astype(np.int64)
    desc = make_desc(offs[frame_of], lens)
    return Batch(name, target, lens, frames, desc, n - nf)


def expected(t: Table, batches, capacity=None):
    """(counters, rule_stats) after the batches, from empty: a bincount by rule_id."""
    cap = t.capacity if capacity is None else capacity
    c = np.zeros(1, COUNTERS_DTYPE)
    st = np.zeros(cap, RULE_STAT_DTYPE)
    for b in batches:
        hit = b.target >= 0
        rid = t.rule_id[b.target[hit]]
        st["packets"] += np.bincount(rid, minlength=cap).astype(np.uint64)
        st["bytes"] += _sum_by(rid, b.lens[hit], cap)
        fwd = int((~t.drops[b.target[hit]]).sum())
        c["pkts_in"] += b.n
        c["pkts_parsed"] += b.n
        c["pkts_matched"] += int(hit.sum())
        c["pkts_forwarded"] += fwd
        c["pkts_dropped"] += b.n - fwd
    return c, st


def _sum_by(rid, lens, cap) -> np.ndarray:
    """Exact integer sums of lens by rule_id (bincount's weights are doubles: exact below 2^53)."""
    s = np.bincount(rid, weights=lens.astype(np.float64), minlength=cap)
    assert s.max(initial=0) < 2.0 ** 53
    return s.astype(np.uint64)


def expected_verdict(t: Table, b: Batch) -> np.ndarray:
    """Code and rule bits of every packet's verdict word (flags 0: no neighbour entry is hit)."""
    hit = b.target >= 0
    safe = np.where(hit, b.target, 0)
    code = np.where(~hit, V_DROP_NOMATCH, np.where(t.drops[safe], V_DROP_RULE, V_FWD))
    return (code | np.where(hit, (b.target + 1) << 8, 0)).astype(np.uint32)


# ---- the shapes -------------------------------------------------------------------------------

def sample_rules(t: Table, most: int) -> np.ndarray:
    """Sorted indexes to aim at: all of them, or for a larger table a stride that keeps every
    boundary index, its neighbours, and both actions."""
    if t.nrules <= most:
        return np.arange(t.nrules)
    step = t.nrules // (most - 32) | 1          # odd: alternates dropping and forwarding rules
    near = [v + d for v in t.boundaries().values() for d in (-1, 0, 1)]
    idx = np.concatenate([np.arange(0, t.nrules, step), np.array(near)])
    return np.unique(idx[(idx >= 0) & (idx < t.nrules)])


def _long_set(t: Table, rules: np.ndarray) -> list:
    """The dropping rules of a batch that carry 65535-byte frames: the boundary ones first."""
    rules = np.asarray(rules)
    first = [v for v in t.boundaries().values() if t.drops[v] and v in set(rules.tolist())]
    plain = rules[t.drops[rules] & (rules % 16 != 1)]          # (those keep their 1514)
    rest = [int(v) for v in plain[:: max(1, len(plain) // LONG_RULES)]]
    return list(dict.fromkeys(first + rest))[:LONG_RULES]


def one_rule(t: Table, idx: int, n: int, which: str = "") -> Batch:
    """Every packet on sorted index idx.  A dropping rule sees the three lengths in turn (three
    frames in memory); a forwarding rule's packets own short frames of varying length."""
    target = np.full(n, idx, np.int64)
    i = np.arange(n)
    lens = np.asarray(LENS)[i % 3] if t.drops[idx] else 60 + (i * 7) % 97
    return build(t, f"one:{which or idx}:{n}", target, lens)


def most_for(t: Table, n: int) -> int:
    """The rules a batch of n packets aims at: all of them where every_rule has room for all (four
    packets a rule on average), else a stride of about MOST that still spans the whole table, so
    that every group-by range is hit in its interior and not only the lowest indexes."""
    return 1 << 30 if 4 * t.nrules <= n else MOST


def ordered_rules(t: Table, most: int = 1 << 30) -> np.ndarray:
    """sample_rules with the boundary indexes first, so that short batches reach them too."""
    rules = sample_rules(t, most)
    bnd = np.isin(rules, list(t.boundaries().values()))
    return np.concatenate([rules[bnd], rules[~bnd]])


def every_rule(t: Table, n: int, most: int | None = None) -> Batch:
    """Rule number k of ordered_rules hit (k mod 7) + 1 times, until n packets are out (so a small
    n reaches the first rules only, a large one wraps round), in a shuffled order, each rule with
    its own length.  `most`: most_for(t, n) unless given."""
    rules = ordered_rules(t, most_for(t, n) if most is None else most)
    seq = np.repeat(rules, np.arange(len(rules)) % 7 + 1)
    rng = np.random.default_rng([13, t.nrules, n])
    target = np.resize(seq, n)[rng.permutation(n)]
    lens = rule_len(t, target, _long_set(t, np.unique(target)))
    return build(t, f"every:{n}", target, lens)


def nothing(t: Table, n: int) -> Batch:
    i = np.arange(n)
    return build(t, f"nothing:{n}", np.full(n, NONE, np.int64), np.asarray(LENS)[i % 3])


def interleaved(t: Table, n: int, most: int | None = None) -> Batch:
    """Matching and non-matching packets within every 64-packet group: two in three match (the
    rules of ordered_rules, in turn), the third matches nothing."""
    rules = ordered_rules(t, most_for(t, n) if most is None else most)
    hit = np.arange(n) % 3 != 2
    target = np.where(hit, rules[(np.cumsum(hit) - 1) % len(rules)], NONE)
    safe = np.where(hit, target, 0)
    lens = np.where(hit, rule_len(t, safe, _long_set(t, np.unique(target[hit]))),
                    np.asarray(LENS)[np.arange(n) % 3])
    return build(t, f"interleaved:{n}", target, lens)


def shapes(t: Table, n: int, most: int | None = None) -> list:
    """Every batch shape over the table at n packets."""
    out = [one_rule(t, idx, n, which) for which, idx in t.boundaries().items()]
    out += [every_rule(t, n, most), nothing(t, n), interleaved(t, n, most)]
    return out


def ranges(t: Table) -> list:
    """(first, end) sorted indexes of the group-by's ranges over the table."""
    return [(r0, min(r0 + K_HIST_RANGE, t.nrules)) for r0 in range(0, t.nrules, K_HIST_RANGE)]


def groups_mixed(b: Batch) -> bool:
    """Every whole 64-packet group holds both a matching and a non-matching packet."""
    hit = b.target >= 0
    whole = b.n // RUN * RUN
    g = hit[:whole].reshape(-1, RUN)
    return bool((g.any(axis=1) & ~g.all(axis=1)).all())


def workload(t: Table, b: Batch) -> synth.Workload:
    arp, ndp = neighbours()
    return synth.Workload(b.name, b.frames, b.desc, t.rules, t.capacity, arp, ndp)


# ---- the 32-bit byte bin -----------------------------------------------------------------------

BYTE_BIN_N = 1 << 20
BYTE_BIN_FRAMES = 64


def byte_bin_batch(t: Table) -> Batch:
    """2^20 descriptors of 65535 bytes over 64 frames in memory, every one on the table's last
    dropping rule: 2^36 bytes less 2^20 on one rule, which a grid of 8 workgroups cannot hold in
    32-bit bins (8 * 2^32 = 2^35) unless the launch is cut."""
    idx = int(np.nonzero(t.drops)[0][-1])
    one = build(t, "frame", np.array([idx]), np.array([LENS[2]]))
    stride = (LENS[2] + 15) // 16 * 16
    frames = np.zeros(BYTE_BIN_FRAMES * stride + len(one.frames) - stride, np.uint8)
    for k in range(BYTE_BIN_FRAMES):
        frames[k * stride:k * stride + 64] = one.frames[:64]
    i = np.arange(BYTE_BIN_N)
    desc = make_desc((i % BYTE_BIN_FRAMES) * stride, np.full(BYTE_BIN_N, LENS[2]))
    return Batch(f"byte-bin:{idx}", np.full(BYTE_BIN_N, idx, np.int64),
                 np.full(BYTE_BIN_N, LENS[2], np.int64), frames, desc,
                 BYTE_BIN_N - BYTE_BIN_FRAMES)

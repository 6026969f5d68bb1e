"""Chosen batches for the segmented calls (upe_gpu_process_segmented and
upe_gpu_process_segmented_resident, upe_amd/csrc/upe_segment.hip): control packets at chosen
places in small batches over chosen tables, each with what the calls must report and what chosen
probe packets must see.  No GPU needed.

A case is a synth.Workload plus what it is named for:

expect     (ctrl, writes, patched, rebuilds) of upe_segment_info_t, written down as the batch is
           laid out (every control packet is added with its effect), not computed from the tables
cuts       the marked packets' positions (the batch is cut behind each)
records    the positions of the packets that carry a record (upe_gpu_ctrl_writes); a record whose
           family has no table is in this list and not in `writes`
probes     (position, "old" | "new" | "none", MAC): a UDP packet to an address some control packet
           of the batch names, and the destination MAC it must leave with — the MAC the tables
           held before the batch, the MAC of the last record before it, or no neighbour at all
filler     the packets that are neither marked nor such a probe (at most half of any batch)

The reference worker keeps a one-entry cache per family in front of each table (L1,
src/worker.c:186-195, 218-225) and a table write does not clear it, so a probe sees a new MAC only
when another destination of its family was forwarded since the last probe to its address: where no
second taught address does that, a packet to a held address that nobody teaches (Y4 / Y6) stands
in between.  Those are the filler.

place:<where>:<new|held>   one ARP learn first, last, in the middle (packet 70 of 130: the second
                           64-packet group), two adjacent, three adjacent of mixed kind, eight
                           control packets and nothing else, a request for the port's own address;
                           the taught addresses absent from the tables, or held under another MAC
norecord:<ns|na|arp|all>   marked packets without a record (an NS without an option, an NA whose
                           option has the NS's type, an ARP with no ARP table) between two packets
                           of one flow; `all`: no marked packet has a record
notable:<arp0|ndp0|both0>  records of a family without a table among records of the other
count:<N>, count:1025:alt  N refresh records over 16 held neighbours, each MAC naming its rank, a
                           probe behind each; alt: every other record teaches a new address
tables:<name>              the tables of tests/neigh_cases.py as the starting tables: records for
                           a reachable entry, each hidden, duplicated and stale address, the zero
                           address where it is held and a new address, twice over, a probe behind
                           each

oracle_run(case)           the restated worker run segment by segment over the stated cuts, so
                           that UPE_VF_L1_INIT is the segmented calls' (relative to each segment's
                           start); everything else equals one run with apply_control
"""
from __future__ import annotations

import dataclasses

import numpy as np

import ctrl_cases as cc
import neigh_cases as nc
import oracle
from upe_amd import synth
from upe_amd.layout import ACT_DROP, ACT_FWD, COUNTERS_DTYPE, RULE_STAT_DTYPE
from upe_amd.synth import _eth, _frame, _ip4, _ip6, _udp

NOW = 1234
PROBE_PORT = 4789
PLACES = ("first", "last", "middle", "adjacent2", "adjacent3", "only8", "port")
FORMS = ("new", "held")
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025)
TABLES = ("hidden", "dup", "stale_head", "wrap", "key0")
SIZES = ("small", "staged", "memory")   # place:* tables: 16 slots, or 4096 around the threshold

SRC4 = 0x0A090001
SRC6 = bytes.fromhex("20010db8000900000000000000000001")
UNTOUCHED = bytes.fromhex("001122334455")    # synth._eth's destination: what a miss leaves


def _v6(k: int) -> bytes:
    return bytes.fromhex("20010db80077") + bytes(8) + k.to_bytes(2, "big")


X4, Z4, Y4 = 0x0A800210, 0x0A800232, 0x0A800221
X6, T6, Y6 = _v6(0x10), _v6(0x32), _v6(0x21)


def mac(tag: int, k: int) -> bytes:
    return bytes([0x02, tag]) + k.to_bytes(4, "big")


OLD = {a: mac(0x01, j) for j, a in enumerate((X4, Z4, Y4, X6, T6, Y6))}


def nd(kind: int, src: bytes, tgt: bytes, opts: bytes = b"") -> bytes:
    """An NS (135: teaches src) or NA (136: teaches tgt) with its options."""
    return _frame(_eth(0x86DD), _ip6(58, src, SRC6, plen=24 + len(opts)),
                  bytes([kind, 0, 0, 0, 0, 0, 0, 0]) + tgt, opts)


def teach(addr, m: bytes, j: int = 0) -> bytes:
    """A control packet that teaches (addr, m): ARP request or reply for an IPv4 address, NS or
    NA for an IPv6 one, by the parity of j."""
    if isinstance(addr, int):
        return cc.arp(1 + j % 2, sha=m, spa=addr)
    if j % 2:
        return nd(136, SRC6, addr, cc.opt(2, m))
    return nd(135, addr, bytes(16), cc.opt(1, m))


def probe_frame(addr, sport: int = 4000) -> bytes:
    if isinstance(addr, int):
        return _frame(_eth(0x0800), _ip4(17, SRC4, addr), _udp(sport, PROBE_PORT), b"\xc3\x3c")
    return _frame(_eth(0x86DD), _ip6(17, SRC6, addr, plen=10), _udp(sport, PROBE_PORT), b"\xc3\x3c")


def rules(total: int = 3) -> np.ndarray:
    """A wildcard FWD rule per family for the probes and IPv4's catch-all DROP; past three, the
    fill rules of neigh_cases.rules (exact 5-tuples no packet here carries) between them."""
    rs = [synth.make_rule(50, ACT_FWD, ip_ver=4, proto=17, dport=PROBE_PORT),
          synth.make_rule(51, ACT_FWD, ip_ver=6, proto=17, dport=PROBE_PORT)]
    tail = synth.rules_array([synth.make_rule(1 << 29, ACT_DROP, ip_ver=4)])
    fill = nc.rules(total + 2)[3:-2] if total > 3 else synth.rules_array([])
    return np.concatenate([synth.rules_array(rs), fill, tail])


@dataclasses.dataclass
class SegCase:
    name: str
    wl: synth.Workload
    expect: tuple
    cuts: tuple
    records: tuple
    probes: tuple
    filler: int
    base: str = ""     # tables:*: the neigh_cases case the tables come from


class _Batch:
    """A batch as it is laid out: every control packet with its effect ("patch", "rebuild",
    "skip": a record without a table, "norecord")."""

    def __init__(self):
        self.items, self.cuts, self.records, self.probes = [], [], [], []
        self.filler = 0
        self.effects = {"patch": 0, "rebuild": 0, "skip": 0, "norecord": 0}

    def ctrl(self, f: bytes, effect: str) -> None:
        self.cuts.append(len(self.items))
        if effect != "norecord":
            self.records.append(len(self.items))
        self.effects[effect] += 1
        self.items.append(f)

    def probe(self, addr, want: str, m=None) -> None:
        self.probes.append((len(self.items), want, m))
        self.items.append(probe_frame(addr))

    def flush(self, addr) -> None:
        """A packet to a held address nobody teaches: the L1 entry of its family moves on."""
        self.filler += 1
        self.items.append(probe_frame(addr, 4001))

    def done(self, name, arp, ndp, n_rules=3, base="") -> SegCase:
        frames, desc = cc.pack([(f, len(f)) for f in self.items])
        e = self.effects
        wl = synth.Workload(name, frames, desc, rules(n_rules), 1024, arp, ndp)
        expect = (len(self.cuts), e["patch"] + e["rebuild"], e["patch"], e["rebuild"])
        return SegCase(name, wl, expect, tuple(self.cuts), tuple(self.records),
                       tuple(self.probes), self.filler, base)


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------

_NEAR: dict = {}


def _near(fam: str) -> np.ndarray:
    """BOUNDARY_N - 8 reachable entries in 4096 slots: eight more still start at a 2048-slot index
    (staged); neigh_cases' boundary_n1 table (BOUNDARY_N + 1) is past it from the start."""
    if fam not in _NEAR:
        _NEAR[fam] = nc._boundary(fam, nc.BOUNDARY_N - 8, seed=1630)
    return _NEAR[fam]


def hold(t: np.ndarray, addr, m: bytes) -> None:
    t["mac"][nc.insert(t, addr)] = np.frombuffer(m, np.uint8)


def tables(held, size: str = "small", caps=(16, 16)):
    """Both families' tables with the addresses of `held` under their OLD MACs."""
    out = []
    for fam, cap in zip(("arp", "ndp"), caps):
        if size == "small":
            t = nc.new_table(fam, cap)
        else:
            t = (_near(fam) if size == "staged" else nc.table(fam, "boundary_n1")).copy()
        for a in held:
            if isinstance(a, int) == (fam == "arp") and len(t):
                hold(t, a, OLD[a])
        out.append(t)
    return out


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------

def _place(where: str, form: str, size: str, n_rules: int) -> SegCase:
    held = form == "held"
    b = _Batch()
    first = "patch" if held else "rebuild"

    def before(a):
        b.probe(a, "old" if held else "none", OLD[a] if held else None)

    def after(a, m, k=1):
        for _ in range(k):
            b.probe(a, "new", m)

    m0, m1, m2 = mac(0x11, 0), mac(0x11, 1), mac(0x11, 2)
    if where == "first":
        b.ctrl(teach(X4, m0), first)
        after(X4, m0, 2)
        b.flush(Y4)
        after(X4, m0, 2)
        b.flush(Y4)
        after(X4, m0)
    elif where == "last":
        for k in (2, 2, 1):
            for _ in range(k):
                before(X4)
            if k == 2:
                b.flush(Y4)
        b.ctrl(teach(X4, m0), first)
    elif where == "middle":
        for _ in range(69):
            before(X4)
        b.flush(Y4)
        b.ctrl(teach(X4, m0), first)
        assert b.cuts == [70]
        after(X4, m0, 2)
        b.flush(Y4)
        after(X4, m0, 56)
    elif where == "adjacent2":
        before(X4)
        b.flush(Y4)
        b.ctrl(teach(X4, m0), first)
        b.ctrl(teach(X4, m1, 1), "patch")
        after(X4, m1)
        b.flush(Y4)
        after(X4, m1, 2)
    elif where == "adjacent3":
        for a in (X4, X6, T6):
            before(a)
        b.flush(Y4)
        b.flush(Y6)
        b.ctrl(teach(X4, m0), first)
        b.ctrl(teach(X6, m1, 0), first)
        b.ctrl(teach(T6, m2, 1), first)
        for a, m in ((X4, m0), (X6, m1), (T6, m2), (X6, m1)):
            after(a, m)
    elif where == "only8":
        for j in range(4):
            b.ctrl(teach(X4, mac(0x12, j), j), first if j == 0 else "patch")
            b.ctrl(teach(X6, mac(0x13, j), j), first if j == 0 else "patch")
    else:
        assert where == "port"
        before(X4)
        b.flush(Y4)
        # answered in place: sha and spa become the port's, so the record is the bytes before
        b.ctrl(cc.arp(1, sha=m0, spa=X4, tpa=synth.PORT_IP4) + bytes(18), first)
        after(X4, m0, 2)
        b.flush(Y4)
        after(X4, m0, 2)
    arp, ndp = tables((Y4, Y6) + ((X4, Z4, X6, T6) if held else ()), size)
    name = f"place:{where}:{form}" + (f":{size}" if size != "small" else "")
    return b.done(name, arp, ndp, n_rules)


def _norecord(which: str) -> SegCase:
    b = _Batch()
    held = (X4, Y4, X6, T6, Y6)
    m0, m1 = mac(0x21, 0), mac(0x21, 1)
    caps = (16, 16)
    if which == "all":
        b.probe(X6, "old", OLD[X6])
        b.ctrl(nd(135, X6, bytes(16)), "norecord")
        b.probe(X6, "old", OLD[X6])
        b.probe(T6, "old", OLD[T6])
        b.ctrl(nd(136, SRC6, T6, cc.opt(1, m0)), "norecord")
        b.probe(T6, "old", OLD[T6])
        b.ctrl(nd(135, X6, bytes(16), cc.opt(2, m1)), "norecord")
        b.ctrl(nd(136, SRC6, T6), "norecord")
    elif which == "arp":
        caps, held = (0, 16), (X6, Y6)
        b.probe(X6, "old", OLD[X6])
        b.ctrl(teach(X4, m0), "skip")
        b.probe(X6, "old", OLD[X6])
        b.flush(Y6)
        b.ctrl(teach(X6, m1), "patch")
        b.probe(X6, "new", m1)
        b.probe(X4, "none")
        b.probe(X6, "new", m1)
    else:
        a = X6 if which == "ns" else T6
        marked = nd(135, X6, bytes(16)) if which == "ns" else nd(136, SRC6, T6, cc.opt(1, m0))
        b.probe(a, "old", OLD[a])
        b.ctrl(marked, "norecord")
        b.probe(a, "old", OLD[a])
        b.flush(Y6)
        b.ctrl(teach(a, m1, which == "na"), "patch")
        for _ in range(3):
            b.probe(a, "new", m1)
    arp, ndp = tables(held, caps=caps)
    return b.done(f"norecord:{which}", arp, ndp)


def flow_pair(c: SegCase):
    """A norecord case's two flow packets around its first marked packet: (first, marked,
    second)."""
    k = c.cuts[0]
    return k - 1, k, k + 1


def _notable(which: str) -> SegCase:
    b = _Batch()
    m = [mac(0x31, j) for j in range(4)]
    if which == "arp0":
        caps, held = (0, 16), (X6, Y6)
        b.probe(X6, "old", OLD[X6])
        b.flush(Y6)
        b.ctrl(teach(X4, m[0]), "skip")
        b.ctrl(teach(X6, m[1]), "patch")
        b.probe(X6, "new", m[1])
        b.probe(X4, "none")
        b.ctrl(teach(X4, m[2], 1), "skip")
        b.ctrl(teach(T6, m[3], 1), "rebuild")
        b.probe(T6, "new", m[3])
        b.probe(X4, "none")
    elif which == "ndp0":
        caps, held = (16, 0), (X4, Y4)
        b.probe(X4, "old", OLD[X4])
        b.flush(Y4)
        b.ctrl(teach(X6, m[0]), "skip")
        b.ctrl(teach(X4, m[1]), "patch")
        b.probe(X4, "new", m[1])
        b.probe(X6, "none")
        b.ctrl(teach(T6, m[2], 1), "skip")
        b.ctrl(teach(Z4, m[3], 1), "rebuild")
        b.probe(Z4, "new", m[3])
        b.probe(X6, "none")
    else:
        assert which == "both0"
        caps, held = (0, 0), ()
        for j, a in enumerate((X4, X6, T6)):
            b.probe(a, "none")
            b.ctrl(teach(a, m[j], j == 2), "skip")
            if j == 0:
                b.probe(a, "none")
        b.ctrl(teach(X4, m[3], 1), "skip")
    arp, ndp = tables(held, caps=caps)
    return b.done(f"notable:{which}", arp, ndp)


HELD16 = tuple(0x0A810000 + 0x0101 * (r + 1) for r in range(16))


def _count(n: int, alt: bool) -> SegCase:
    """Record j refreshes HELD16[j % 16] with a MAC that names j; alt: the odd records teach new
    addresses instead (512 of them in 1024 slots)."""
    b = _Batch()
    for j in range(n):
        m = mac(0xC0, j)
        if alt and j % 2:
            a, effect = 0x0A900000 + j, "rebuild"
        else:
            a, effect = HELD16[(j // 2 if alt else j) % 16], "patch"
        b.ctrl(teach(a, m, j), effect)
        b.probe(a, "new", m)
    arp = nc.new_table("arp", 1024 if alt else 64)
    for r, a in enumerate(HELD16):
        hold(arp, a, mac(0x20, r))
    ndp = tables((Y6,))[1]
    return b.done(f"count:{n}" + (":alt" if alt else ""), arp, ndp)


def table_targets(fam: str, small: str):
    """[(address, effect of its first record)] for a neigh_cases table, by its anatomy: a write to
    an address the reference's probe reaches is a refresh, any other inserts."""
    an = nc.anatomy(nc.table(fam, small))
    zero = nc.ZERO[fam]
    plain = [k for k in an["reachable"] if k not in an["dup"] and k != zero]
    out = [(plain[0], "patch")]
    out += [(k, "rebuild") for k in an["hidden"]]
    out += [(k, "patch") for k in an["dup"]]
    out += [(k, "rebuild") for k in an["stale"]]
    if zero in an["reachable"]:
        out.append((zero, "patch"))
    out.append((nc.homed(fam, 16, 9, 900), "rebuild"))
    return out


def _tables(name: str) -> SegCase:
    base = name[len("tables:"):]
    cs = nc.case(base)
    small = base.split(":")[-1]
    t4, t6 = table_targets("arp", small), table_targets("ndp", small)
    assert len(t4) == len(t6)
    b = _Batch()
    for rnd in range(2):
        for j in range(len(t4)):
            for f, (a, effect) in enumerate((t4[j], t6[j])):
                m = mac(0xE0 + 4 * rnd + f, j)
                b.ctrl(teach(a, m, j + rnd), effect if rnd == 0 else "patch")
                b.probe(a, "new", m)
    return b.done(name, cs.arp.copy(), cs.ndp.copy(), base=base)


ALL = ([f"place:{w}:{f}" for w in PLACES for f in FORMS] +
       [f"norecord:{w}" for w in ("ns", "na", "arp", "all")] +
       [f"notable:{w}" for w in ("arp0", "ndp0", "both0")] +
       [f"count:{n}" for n in COUNTS] + ["count:1025:alt"] +
       [f"tables:{p}{t}" for p in ("", "embed:") for t in TABLES])
_CASES: dict = {}


def case(name: str, n_rules: int = 3) -> SegCase:
    """A case by name, built once.  "place:<where>:<form>:<staged|memory>": the same batch over
    4096-slot tables on either side of the staging threshold."""
    if (name, n_rules) not in _CASES:
        p = name.split(":")
        if p[0] == "place":
            c = _place(p[1], p[2], p[3] if len(p) > 3 else "small", n_rules)
        elif p[0] == "norecord":
            c = _norecord(p[1])
        elif p[0] == "notable":
            c = _notable(p[1])
        elif p[0] == "count":
            c = _count(int(p[1]), len(p) > 2)
        else:
            assert p[0] == "tables"
            c = _tables(name)
        if n_rules != 3:
            c.wl.rules = rules(n_rules)
        for a in (c.wl.frames, c.wl.desc, c.wl.arp, c.wl.ndp):
            a.setflags(write=False)
        _CASES[name, n_rules] = c
    return _CASES[name, n_rules]


def without(c: SegCase, i: int) -> SegCase:
    """The case's batch with packet i (a marked packet) taken out: the cuts behind it move up."""
    assert i in c.cuts
    keep = np.arange(c.wl.n) != i
    wl = dataclasses.replace(c.wl, desc=c.wl.desc[keep].copy())
    cuts = tuple(k - (k > i) for k in c.cuts if k != i)
    return dataclasses.replace(c, wl=wl, cuts=cuts)


# ---------------------------------------------------------------------------------------------
# the oracle, segment by segment
# ---------------------------------------------------------------------------------------------

def oracle_run(c: SegCase, start: oracle.Result | None = None) -> oracle.Result:
    """The restated worker over the batch, one call per segment (up to and including each stated
    cut, then the rest), tables, L1, counters and rule_stats carried: what the segmented calls
    must give, UPE_VF_L1_INIT included.  start: a Result to continue from (its tables, L1,
    counters and rule_stats; the frames start afresh)."""
    wl = c.wl
    lib = oracle.oracle_lib()
    ptr = oracle._ptr
    rs = np.ascontiguousarray(wl.rules_sorted)
    frames, desc = wl.frames.copy(), np.ascontiguousarray(wl.desc)
    if start is None:
        arp, ndp, l1 = wl.arp.copy(), wl.ndp.copy(), wl.l1.copy()
        cnt, st = np.zeros(1, COUNTERS_DTYPE), np.zeros(wl.capacity, RULE_STAT_DTYPE)
    else:
        arp, ndp, l1 = start.arp.copy(), start.ndp.copy(), start.l1.copy()
        cnt, st = start.counters.copy(), start.rule_stats.copy()
    verdict = np.zeros(wl.n, np.uint32)
    eth = np.frombuffer(bytes(wl.eth_addr), np.uint8).copy()
    bounds = [0] + [k + 1 for k in c.cuts]
    if bounds[-1] < wl.n:
        bounds.append(wl.n)
    for s, e in zip(bounds[:-1], bounds[1:]):
        d, v = desc[s:e].copy(), np.zeros(e - s, np.uint32)
        rc = lib.upe_ref_process(ptr(rs), len(rs), ptr(arp), len(arp), ptr(ndp), len(ndp), ptr(eth),
                                 wl.ip4_addr, 1, ptr(l1), ptr(frames), ptr(d), e - s, ptr(v),
                                 ptr(cnt), ptr(st), wl.capacity)
        assert rc == 0
        verdict[s:e] = v
    return oracle.Result(frames, verdict, cnt, st, l1, arp, ndp, rs)


_ORACLE: dict = {}


def oracle_of(name: str, n_rules: int = 3) -> oracle.Result:
    """One segmented oracle run per case, shared by the CPU and GPU tests and left unchanged."""
    if (name, n_rules) not in _ORACLE:
        _ORACLE[name, n_rules] = oracle_run(case(name, n_rules))
    return _ORACLE[name, n_rules]

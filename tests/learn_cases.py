"""Control-write records that teach NEW neighbours, for upe_gpu_neigh_learn and its twins
(tests/test_neigh_learn.py, tests/test_gpu_neigh_learn.py): the tables of tests/neigh_cases.py small
and embedded in 8192 slots, a sparse table with thousands of free slots, and record lists made for
each branch of the contract (include/upe_gpu.h).  Every case states the (patched, inserted, dropped,
deferred) it must give and, where it is made to defer, the ranks deferred; tests/test_neigh_learn.py
asserts both against model() below, so that no parity test passes by deferring everything.

model() is the contract written once more, on dictionaries, with its own copy of the index hashes:
it shares no code with upe_neigh_learn_host or neigh.learn."""
from __future__ import annotations

import dataclasses

import numpy as np

import neigh_cases as nc
import patch_cases as pc
import resolve_cases as rc
from upe_amd import gpu
from upe_amd.layout import ARP_DTYPE, CW_ARP, CW_NDP, NDP_DTYPE

M32 = 0xFFFFFFFF
NONE64 = (1 << 64) - 1
COUNTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
BIG_ROOM = 32768   # an index of 2^16 slots: 2049 new addresses keep a free candidate each
KIND = {"arp": CW_ARP, "ndp": CW_NDP}


# ---------------------------------------------------------------------------------------------
# the index hashes (csrc/upe_dev.h), restated
# ---------------------------------------------------------------------------------------------

def _mul(a, b):
    return (a * b) & M32


def candidates(key32: int, seed: int, bits: int):
    s1 = _mul(key32 ^ seed, 0x9E3779B1) >> (32 - bits)
    x = _mul(key32 ^ seed, 0x85EBCA77)
    s2 = _mul(x ^ (x >> 16), 0xC2B2AE3D) >> (32 - bits)
    x = _mul(key32 ^ _mul(seed, 0x9E3779B9), 0x27D4EB2F)
    s3 = _mul(x ^ (x >> 15), 0x165667B1) >> (32 - bits)
    return s1, s2, s3


def key32(fam: str, addr) -> int:
    return int(addr) if fam == "arp" else nc.fold_v6(nc.words("ndp", addr))


# ---------------------------------------------------------------------------------------------
# the sequential model
# ---------------------------------------------------------------------------------------------

def model(index, recs):
    """The contract's loop on (info, arp_slots, ndp_slots) of gpu.NeighImage.read().  Returns
    (index after, deferred ranks, (records, patched, inserted, dropped, deferred, first_defer,
    arp_free, ndp_free), outcome per record: "p" / "i" / "x" / "d")."""
    meta, slots = index[0].copy(), {"arp": index[1].copy(), "ndp": index[2].copy()}
    held = {}   # family -> {slot: address} of the used slots
    for fam, aw, uw in (("arp", 1, 2), ("ndp", 4, 5)):
        s = slots[fam]
        held[fam] = {int(j): s[j, :aw].tobytes() for j in np.nonzero((s[:, uw] >> 16) & 1)[0]}
    free = {f: int(meta[f + "_free"]) for f in ("arp", "ndp")}
    out = []
    for r in range(len(recs)):
        kind = int(recs["kind"][r])
        fam = "arp" if kind == CW_ARP else "ndp" if kind == CW_NDP else None
        if fam is None:
            out.append("d")
            continue
        raw = recs["ip"][r].tobytes()
        addr = raw[:4] if fam == "arp" else raw
        bits, seed = int(meta[fam + "_bits"]), int(meta[fam + "_seed"])
        k = int.from_bytes(addr, "little") if fam == "arp" else nc.fold_v6(nc.words("ndp", addr))
        cand = candidates(k, seed, bits) if bits else ()
        mac = recs["mac"][r].tobytes()
        lo, hi = int.from_bytes(mac[:4], "little"), int.from_bytes(mac[4:], "little")
        s, m = slots[fam], 1 if fam == "arp" else 4
        at = next((c for c in cand if held[fam].get(c) == addr), None)
        if at is not None:
            s[at, m], s[at, m + 1] = lo, (int(s[at, m + 1]) & 0xFFFF0000) | hi
            out.append("p")
        elif not int(meta[fam + "_insertable"]):
            out.append("d")
        elif free[fam] == 0:
            out.append("x")
        else:
            at = next((c for c in cand if c not in held[fam]), None)
            if at is None:
                out.append("d")
                continue
            s[at] = 0
            s[at, :m] = np.frombuffer(addr, "<u4")
            s[at, m], s[at, m + 1] = lo, hi | 0x10000
            held[fam][at] = addr
            free[fam] -= 1
            out.append("i")
    meta["arp_free"], meta["ndp_free"] = free["arp"], free["ndp"]
    defer = np.array([r for r, o in enumerate(out) if o == "d"], np.uint32)
    info = (len(recs), out.count("p"), out.count("i"), out.count("x"), len(defer),
            int(defer[0]) if len(defer) else NONE64, free["arp"], free["ndp"])
    return (meta, slots["arp"], slots["ndp"]), defer, info, out


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass
class LearnCase:
    name: str
    arp: np.ndarray
    ndp: np.ndarray
    room: "tuple | None"
    recs: np.ndarray
    expect: tuple           # (patched, inserted, dropped, deferred)
    defer: "list | None"    # the ranks that must be deferred; None: a case named for insertion
    base: str = ""          # the neigh_cases table behind it, if any (its queries join the keys)

    def image(self) -> "gpu.NeighImage":
        return gpu.NeighImage(self.arp, self.ndp, room=self.room)


def fresh(fam: str, tag: int):
    """A new address: none of the case tables, the sparse one or another tag holds it."""
    if fam == "arp":
        return 0xC6000000 | (tag * 0x9E5 + 7) & 0xFFFFFF
    return bytes([0xFD, 0x5E]) + int(tag * 0x9E3779B1 + 11).to_bytes(8, "big") + bytes(6)


def sparse(fam: str) -> np.ndarray:
    """4096 slots, 8 entries: room in the table for every burst of COUNTS."""
    t = nc.new_table(fam, 4096)
    for j in range(8):
        nc.insert(t, nc.homed(fam, 4096, 37 * j + 5, j + 1))
    return t


def _tables(name: str):
    if name == "sparse":
        return sparse("arp"), sparse("ndp")
    return nc.table("arp", name), nc.table("ndp", name)


def _room(t) -> tuple:
    """Room that leaves each index sparse enough for a handful of new addresses to find a free
    candidate each: the embedded tables' indexes hold 1700 entries."""
    return (8192, 8192) if len(t) > 64 else (64, 64)


def _reach(t) -> list:
    return list(nc.anatomy(t)["reachable"])


def _both(tag0: int, n: int) -> list:
    """n new addresses per family, alternating."""
    out = []
    for j in range(n):
        out += [(CW_ARP, fresh("arp", tag0 + j)), (CW_NDP, fresh("ndp", tag0 + j))]
    return out


def _filled(fam: str, free: int) -> np.ndarray:
    """8 slots, `free` of them invalid, every entry reachable."""
    t = nc.new_table(fam, 8)
    for j in range(8 - free):
        nc.insert(t, nc.homed(fam, 8, (3 * j) % 8, j + 1))
    return t


def _search(index, fam: str, want, tag0: int = 5000, limit: int = 200000):
    """The first new address of `fam` (tags upward from tag0) whose candidate slots satisfy
    want(candidates)."""
    meta = index[0]
    bits, seed = int(meta[fam + "_bits"]), int(meta[fam + "_seed"])
    for tag in range(tag0, tag0 + limit):
        a = fresh(fam, tag)
        if want(candidates(key32(fam, a), seed, bits)):
            return a, tag
    raise AssertionError("no such address")


def _used(index, fam: str) -> set:
    s, uw = (index[1], 2) if fam == "arp" else (index[2], 5)
    return {int(j) for j in np.nonzero((s[:, uw] >> 16) & 1)[0]}


def _build(name: str) -> LearnCase:
    kind, _, arg = name.partition(":")
    if kind == "one_new":
        a, n = _tables(arg)
        return LearnCase(name, a, n, _room(a), pc.make(_both(1, 1)), (0, 2, 0, 0), None, arg)
    if kind == "twice":      # the later MAC wins: the second record refreshes what the first put in
        a, n = _tables(arg)
        items = _both(3, 1) + _both(3, 1)
        return LearnCase(name, a, n, _room(a), pc.make(items), (2, 2, 0, 0), None, arg)
    if kind == "interleaved":
        a, n = _tables(arg)
        old = [(CW_ARP, k) for k in _reach(a)[:6]] + [(CW_NDP, k) for k in _reach(n)[:6]]
        new = _both(10, len(old) // 2 + 1)
        items = [x for pair in zip(new, old) for x in pair] + new[len(old):] + old[:2]
        return LearnCase(name, a, n, _room(a), pc.make(items), (len(old) + 2, len(new), 0, 0),
                         None, arg)
    if kind == "zero":       # 0.0.0.0 and :: are ordinary addresses to the tables
        a, n = _tables(arg)
        items = [(CW_ARP, 0), (CW_NDP, bytes(16)), (CW_ARP, 0)]
        return LearnCase(name, a, n, _room(a), pc.make(items), (1, 2, 0, 0), None, arg)
    if kind == "free":       # exactly `free` invalid slots against three new addresses per family
        free = int(arg)
        items = _both(20, 3) + _both(20, 1)   # the first address again, last
        took = min(free, 3)
        # the repeat: a refresh where its address got in, dropped with the rest otherwise
        again = 2 if took >= 1 else 0
        return LearnCase(name, _filled("arp", free), _filled("ndp", free), (64, 64), pc.make(items),
                         (again, 2 * took, 2 * (3 - took) + 2 - again, 0), None)
    if kind == "no_table":   # the ARP family has no table
        a, n = nc.new_table("arp", 0), nc.table("ndp", "wrap")
        items = _both(30, 2)
        if arg == "room":    # a real index with no slot used and nothing free: dropped
            return LearnCase(name, a, n, (64, 64), pc.make(items), (0, 2, 2, 0), None)
        return LearnCase(name, a, n, (0, 64), pc.make(items), (0, 2, 0, 2), [0, 2])
    if kind == "unreached":  # an entry no probe reaches: nothing new may go in
        a, n = _tables(arg)
        old = [(CW_ARP, k) for k in _reach(a)[:2]] + [(CW_NDP, k) for k in _reach(n)[:2]]
        items = old + _both(40, 3) + [(0, 1), (5, 2)]
        nd = 6 + 2
        return LearnCase(name, a, n, _room(a), pc.make(items), (len(old), 0, 0, nd),
                         list(range(len(old), len(items))), arg)
    if kind == "one_fold4":  # four new addresses of one fold_v6: the fourth has no candidate left
        a, n = _tables("sparse")
        first = fresh("ndp", 50)
        same = [first] + [nc.same_fold(first, 7 * j, j, 0x50 + j) for j in (1, 2, 3)]
        assert len({nc.fold_v6(nc.words("ndp", x)) for x in same}) == 1 and len(set(same)) == 4
        items = [(CW_NDP, x) for x in same] + [(CW_NDP, same[1])]
        return LearnCase(name, a, n, (64, 64), pc.make(items), (1, 3, 0, 1), [3])
    if kind == "cands_used":  # an address whose three candidates are all used, found by search
        a, n = _tables("embed:wrap")
        index = gpu.NeighImage(a, n).read()
        items = []
        for fam in ("arp", "ndp"):
            used = _used(index, fam)
            full, _ = _search(index, fam, lambda c: all(x in used for x in c))
            ok, _ = _search(index, fam, lambda c: c[0] in used and c[1] not in used, 9000)
            items += [(KIND[fam], ok), (KIND[fam], full)]
        return LearnCase(name, a, n, None, pc.make(items), (0, 2, 0, 2), [1, 3], "embed:wrap")
    if kind == "count":      # n new records against an image compiled with room
        a, n = _tables("sparse")
        items = _both(100, (int(arg) + 1) // 2)[:int(arg)]
        return LearnCase(name, a, n, (BIG_ROOM, BIG_ROOM), pc.make(items, salt=0x33),
                         (0, int(arg), 0, 0), None)
    if kind == "shared_first":
        # every address after the first has a first candidate that a lower rank takes: its first
        # bid loses, and some lose twice
        a, n = _tables("sparse")
        index = gpu.NeighImage(a, n, room=(64, 64)).read()
        items = []
        for fam in ("arp", "ndp"):
            bits, seed = int(index[0][fam + "_bits"]), int(index[0][fam + "_seed"])
            taken, tag, mine = _used(index, fam), 7000, 0
            while mine < 20:
                addr, tag = _search(index, fam, lambda c: not mine or (
                    c[0] in taken and any(x not in taken for x in c)), tag + 1)
                c = candidates(key32(fam, addr), seed, bits)
                taken.add(next(x for x in c if x not in taken))
                items.append((KIND[fam], addr))
                mine += 1
        order = [x for pair in zip(items[:20], items[20:]) for x in pair]
        return LearnCase(name, a, n, (64, 64), pc.make(order, salt=0x44), (0, 40, 0, 0), None)
    raise KeyError(name)


BASES = ("wrap", "embed:wrap", "key0", "embed:key0")
CASES = ([f"{k}:{t}" for k in ("one_new", "twice", "interleaved") for t in BASES + ("sparse",)] +
         ["zero:no_key0", "zero:embed:no_key0", "free:0", "free:1", "free:2", "no_table:",
          "no_table:room", "unreached:hidden", "unreached:embed:hidden", "unreached:combo",
          "one_fold4:", "cands_used:", "shared_first:"] +
         [f"count:{n}" for n in COUNTS])
_CASES: dict = {}


def case(name: str) -> LearnCase:
    """A case, built once (read-only)."""
    if name not in _CASES:
        c = _build(name)
        for x in (c.arp, c.ndp, c.recs):
            x.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def keys(c: LearnCase) -> np.ndarray:
    """(n, 44) key records: every address the tables store, every record's address (in its kind's
    family), the base case's queries, and absent addresses."""
    rng = np.random.default_rng([0x1EA2] + list(c.name.encode()))
    fams, addrs = [], []
    for fam, t in (("arp", c.arp), ("ndp", c.ndp)):
        st = nc.stored(t)
        if len(st) > 300:
            st = [st[int(j)] for j in rng.permutation(len(st))[:300]]
        fams += [fam] * len(st)
        addrs += st
        fams += [fam] * 16
        addrs += [nc._random_key(fam, rng) for _ in range(16)]
    parts = [rc.key_bytes(fams, addrs, rng), pc.record_keys(c.recs, rng)]
    if c.base and c.base != "sparse":
        parts.append(rc.queries(c.base)[0])
    return np.concatenate(parts)


def applied(c: LearnCase, defer) -> tuple:
    """The case's slot arrays after upe_neigh_apply_writes of the records that are not deferred."""
    keep = np.ones(len(c.recs), bool)
    keep[np.asarray(defer, np.int64)] = False
    a, n = c.arp.copy(), c.ndp.copy()
    known = np.isin(c.recs["kind"], (CW_ARP, CW_NDP))
    gpu.neigh_apply_writes(a, n, c.recs[keep & known], now=77)
    return a, n

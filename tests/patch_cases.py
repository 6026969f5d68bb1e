"""Control-write records over the neighbour tables of tests/neigh_cases.py, for the refresh on the
device (upe_gpu_neigh_patch) and its twins (tests/test_neigh_patch.py, tests/test_gpu_neigh_patch.py).

A case's records, the two families alternating: every address stored anywhere in the slot arrays
(of a large table: the case's own and a seeded sample) with a MAC of its own — so the reachable ones
are refreshed and each kind a probe does not reach is aimed at: an entry behind an invalid slot, a
stale address in an invalid slot, the second of two slots holding one address (the first answers
and is rewritten; the second keeps its MAC); one reachable address of each family three more times
(the last must win); absent addresses, 0.0.0.0 and :: among them; records of no kind.  A MAC names
its record's rank, so which record a slot's MAC came from can be read off it."""
from __future__ import annotations

import numpy as np

import neigh_cases as nc
import resolve_cases as rc
from upe_amd.layout import CTRL_WRITE_DTYPE, CW_ARP, CW_NDP

CASES = nc.SMALL_CASES + nc.MEMORY_CASES
SAMPLE = 300   # addresses of a large table that get a record
ABSENT = 64
_RECORDS: dict = {}


def rank_mac(rank: int, salt: int = 0) -> bytes:
    return bytes([0x0A, salt & 0xFF, (rank >> 16) & 0xFF, (rank >> 8) & 0xFF, rank & 0xFF, 0x5C])


def make(items, salt: int = 0) -> np.ndarray:
    """[(kind, address)] -> records in that order: index 3 * rank + 1, mac rank_mac(rank)."""
    w = np.zeros(len(items), CTRL_WRITE_DTYPE)
    for r, (kind, a) in enumerate(items):
        w["index"][r] = 3 * r + 1
        w["kind"][r] = kind
        w["mac_off"][r] = 22
        w["mac"][r] = np.frombuffer(rank_mac(r, salt), np.uint8)
        b = int(a).to_bytes(4, "little") + bytes(12) if isinstance(a, (int, np.integer)) else a
        w["ip"][r] = np.frombuffer(b, np.uint8)
    return w


def _family_items(cs: nc.Case, fam: str, rng) -> list:
    kind = CW_ARP if fam == "arp" else CW_NDP
    t = cs.table(fam)
    st, own = nc.stored(t), cs.own(fam)
    if len(st) > SAMPLE:
        rest = [k for k in st if k not in set(own)]
        st = own + [rest[int(j)] for j in rng.permutation(len(rest))[:SAMPLE - len(own)]]
    out = [(kind, k) for k in st]
    probe = nc.Probe(t)
    reach = [k for k in st if probe.slot(k) >= 0]
    if reach:
        out += [(kind, reach[len(reach) // 2])] * 3
    absent = [nc.ZERO[fam]] + [nc._random_key(fam, rng) for _ in range(ABSENT // 2 - 1)]
    out += [(kind, k) for k in absent]
    out += [(0, st[0] if st else nc.ZERO[fam]), (5, absent[1])]   # records of no kind
    return out


def records(name: str) -> np.ndarray:
    """The case's records, built once (read-only)."""
    if name not in _RECORDS:
        cs = nc.case(name)
        rng = np.random.default_rng([0x9A7C] + list(name.encode()))
        a, b = _family_items(cs, "arp", rng), _family_items(cs, "ndp", rng)
        items = []
        for j in range(max(len(a), len(b))):
            items += ([a[j]] if j < len(a) else []) + ([b[j]] if j < len(b) else [])
        w = make(items)
        w.setflags(write=False)
        _RECORDS[name] = w
    return _RECORDS[name]


def record_keys(w: np.ndarray, rng=None) -> np.ndarray:
    """(n, 44) key records asking for each record's address in its kind's family (ip_ver = kind;
    a record of no kind asks nothing)."""
    rng = rng or np.random.default_rng(5)
    fams = [int(k) for k in w["kind"]]
    addrs = [int.from_bytes(bytes(ip[:4]), "little") if k == CW_ARP else bytes(ip)
             for k, ip in zip(fams, w["ip"])]
    return rc.key_bytes(fams, addrs, rng)


def address_keys(name: str, w: np.ndarray) -> np.ndarray:
    """Keys for every address of the case's tables (its queries: stored, flipped, zero, random),
    every record's address, and ABSENT more absent ones."""
    rng = np.random.default_rng([0xADD5] + list(name.encode()))
    extra = rc.key_bytes(["arp", "ndp"] * (ABSENT // 2),
                         [nc._random_key(f, rng) for f in ["arp", "ndp"] * (ABSENT // 2)], rng)
    return np.concatenate([rc.queries(name)[0], record_keys(w, rng), extra])


def held(arp, ndp, w: np.ndarray) -> np.ndarray:
    """Which records' addresses the reference's probe reaches in the slot arrays (the pinned probe
    model, neigh_cases.Probe), by kind."""
    p = {CW_ARP: nc.Probe(arp), CW_NDP: nc.Probe(ndp)}
    out = np.zeros(len(w), bool)
    for r in range(len(w)):
        k = int(w["kind"][r])
        if k in p:
            ip = bytes(w["ip"][r])
            out[r] = p[k].slot(int.from_bytes(ip[:4], "little") if k == CW_ARP else ip) >= 0
    return out

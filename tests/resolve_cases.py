"""Flow keys that ask the neighbour tables of tests/neigh_cases.py for next hops, for the CPU twins
(tests/test_resolve.py) and the device call (tests/test_gpu_resolve.py).

A case's queries, per family, in three groups: the case's own addresses (an embedded table's are
the small table's), every address stored anywhere in the slot array (invalid slots' too), and
stored addresses with one bit flipped that are stored nowhere (same chain, or the next); then the
all-zero address and a few random ones.  The two families alternate key by key as far as both
last.  Keys are built as bytes: everything upe_gpu_resolve_keys must not read (the padding, the
source address, ports and protocol, an IPv4 key's union bytes 4-15) is filled with noise.
"""
from __future__ import annotations

import numpy as np

import neigh_cases as nc
from upe_amd.layout import FLOW_KEY_DTYPE

CASES = nc.SMALL_CASES + nc.MEMORY_CASES + nc.BOUNDARY_CASES
FOUND = 1 << 48
_QUERIES: dict = {}


def key_bytes(fams, addrs, rng, clean4: bool = False) -> np.ndarray:
    """(n, 44) key records: fams[i] = "arp" / "ndp" / an ip_ver number, addrs[i] = an int (IPv4,
    host order), 16 bytes, or None.  Noise everywhere else, also behind an IPv4 address unless
    clean4."""
    n = len(fams)
    kb = rng.integers(0, 256, size=(n, 44), dtype=np.uint8)
    for i, (f, a) in enumerate(zip(fams, addrs)):
        kb[i, 0] = 4 if f == "arp" else 6 if f == "ndp" else f
        if isinstance(a, (int, np.integer)):
            kb[i, 20:24] = np.frombuffer(int(a).to_bytes(4, "little"), np.uint8)
            if clean4:
                kb[i, 24:36] = 0
        elif a is not None:
            kb[i, 20:36] = np.frombuffer(a, np.uint8)
    return kb


def as_keys(kb: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(kb).view(FLOW_KEY_DTYPE).ravel()


def family_queries(cs: nc.Case, fam: str, rng):
    """[(group, address)] of one family."""
    t = cs.table(fam)
    own, st = cs.own(fam), nc.stored(t)
    held = set(st)
    out = [("own", k) for k in own] + [("stored", k) for k in st]
    src = own * 4 + st
    want = 0 if not src else max(24, min(4 * len(src), 256))
    seen = set()
    while want > 0:
        k = nc._flip(fam, src[int(rng.integers(0, len(src)))], rng)
        if k not in held and k not in seen:
            seen.add(k)
            out.append(("flip", k))
            want -= 1
    out.append(("zero", nc.ZERO[fam]))
    out += [("random", nc._random_key(fam, rng)) for _ in range(8)]
    return out


def queries(name: str):
    """(key bytes (n, 44), families, addresses, groups) of a case, built once."""
    if name not in _QUERIES:
        cs = nc.case(name)
        rng = np.random.default_rng([0x7E5] + list(name.encode()))
        q4, q6 = family_queries(cs, "arp", rng), family_queries(cs, "ndp", rng)
        fams, addrs, groups = [], [], []
        for j in range(max(len(q4), len(q6))):
            for fam, q in (("arp", q4), ("ndp", q6)):
                if j < len(q):
                    fams.append(fam)
                    groups.append(q[j][0])
                    addrs.append(q[j][1])
        kb = key_bytes(fams, addrs, rng)
        kb.setflags(write=False)
        _QUERIES[name] = (kb, fams, addrs, groups)
    return _QUERIES[name]


def mac_word(mac) -> int:
    """A probe's answer (6 bytes or None) in upe_gpu_resolve_keys' format."""
    return 0 if mac is None else int.from_bytes(mac, "little") | FOUND


def probe_words(cs: nc.Case, fams, addrs) -> np.ndarray:
    """The pinned probe model's answers (neigh_cases.Probe, checked against the reference by
    tests/test_neigh_cases.py), one uint64 per key."""
    p = {"arp": nc.Probe(cs.arp), "ndp": nc.Probe(cs.ndp)}
    return np.array([mac_word(p[f].mac(a)) for f, a in zip(fams, addrs)], np.uint64)

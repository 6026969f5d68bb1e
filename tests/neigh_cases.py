"""Adversarial neighbour tables and the traffic that reaches them.

The GPU path answers arp_get_mac / ndp_get_mac (reference src/arp_table.c:55-80,
src/ndp_table.c:67-86) from a three-choice cuckoo index that build_neigh_image
(upe_amd/csrc/upe_rules.cpp) builds from the reference's linear-probe slot arrays.  synth.arp_table
/ synth.ndp_table only make arrays a learned table would hold right after its inserts; the slot
arrays here are written slot by slot (put), so that they hold what expiry, wrap-around and
re-learning leave behind: entries no probe reaches, one address in two slots, stale addresses in
invalid slots, a valid entry for 0.0.0.0 / ::, addresses that share the index's 32-bit key
(fold_v6) or the reference's home slot.  tools/neigh_san.cpp runs the same shapes through the host
builder alone; these go through the kernels (tests/test_gpu_neigh_tables.py) after
tests/test_neigh_cases.py has pinned, on the CPU, that each does what its name says.

An ARP address is an int (host order, as arp_entry_t.ip), an NDP address 16 wire bytes.  The
family of a table is its dtype's.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from keyframes import arrange_runs, canonical, frames_from_keys
from upe_amd import synth
from upe_amd.layout import (ACT_DROP, ACT_FWD, ARP_DTYPE, FLOW_KEY_DTYPE, NDP_DTYPE, RULE_DTYPE,
                            desc_lens, desc_offsets, make_desc)

N_PACKETS = 4096 + 37   # a ragged last chunk
BIG = 8192              # slots of an embedding table
FILLERS = 1700          # its ordinary entries: 5 * 1700 > 4 * 2048, so the index takes 4096 slots
CLEAR = 24              # slots at either end of an embedding table that the fillers leave alone
# cuckoo3_place starts at the least 2^bits with 4 * 2^bits >= 5 n: 1638 reachable entries are the
# most that start at 2048 slots (the largest staged index), 1639 start at 4096 (read from memory)
BOUNDARY_N = 1638
M32 = 0xFFFFFFFF
ZERO = {"arp": 0, "ndp": bytes(16)}
NDP_ONLY = ("one_fold", "one_home")
PORT_DROP_D, PORT_DROP_S, PORT_ACTION = 7001, 7002, 7003


# ---------------------------------------------------------------------------------------------
# addresses
# ---------------------------------------------------------------------------------------------

def family(table: np.ndarray) -> str:
    return "arp" if table.dtype == ARP_DTYPE else "ndp"


def new_table(fam: str, cap: int) -> np.ndarray:
    return np.zeros(cap, ARP_DTYPE if fam == "arp" else NDP_DTYPE)


def words(fam: str, key) -> tuple:
    """An address as four words: ARP word 0 = the address, NDP the 16 bytes as LE words."""
    if fam == "arp":
        return (int(key), 0, 0, 0)
    return tuple(int.from_bytes(key[4 * j:4 * j + 4], "little") for j in range(4))


def from_words(fam: str, w) -> "int | bytes":
    if fam == "arp":
        return int(w[0]) & M32
    return b"".join((int(x) & M32).to_bytes(4, "little") for x in w)


def home(fam: str, key, cap: int) -> int:
    """The slot a probe of `key` starts at: ARP the address's low bits (src/arp_table.c:30),
    NDP the XOR of the four LE words (ndp_hash, src/ndp_table.c:6-17; synth.ndp_hash)."""
    w = words(fam, key)
    return (w[0] ^ w[1] ^ w[2] ^ w[3]) & (cap - 1)


def fold_v6(w) -> int:
    """upe_dev.h fold_v6: the 32-bit key the NDP index places an address by."""
    return ((w[0] * 0x9E3779B1) ^ (w[1] * 0x85EBCA77) ^ (w[2] * 0xC2B2AE3D) ^
            (w[3] * 0x27D4EB2F)) & M32


FOLD_INV = pow(0x9E3779B1, -1, 1 << 32)   # fold_v6 multiplies word 0 by an odd constant


def same_fold(a, w1: int, w2: int, w3: int) -> bytes:
    """The NDP address with words 1-3 as given whose fold_v6 equals that of address `a`."""
    rest = fold_v6((0, w1 & M32, w2 & M32, w3 & M32))
    w0 = ((fold_v6(words("ndp", a)) ^ rest) * FOLD_INV) & M32
    return from_words("ndp", (w0, w1, w2, w3))


def _ext(cap: int, h: int) -> int:
    """Home slot h of a `cap`-slot table as 16 low bits that name the same place in every larger
    table (embed): the lower half of the table counts up from slot 0, the upper half down from
    the last slot."""
    return h if h < cap // 2 else h | (0xFFFF & ~(cap - 1))


def homed(fam: str, cap: int, h: int, tag: int):
    """An address whose home slot in a table of `cap` slots is `h`; `tag` tells addresses of one
    home apart.  (Its home in a larger table is `h` counted from the same end, see embed.)"""
    assert 0 <= h < cap <= 1 << 16 and 0 <= tag < 1 << 15
    w = [0, tag << 8, (tag * 0x01010101) & M32, 0] if fam == "ndp" else [0, 0, 0, 0]
    w[0] = ((tag + 1) << 16) | _ext(cap, h)
    w[0] ^= (w[1] ^ w[2] ^ w[3]) & 0xFFFF
    return from_words(fam, w)


# ---------------------------------------------------------------------------------------------
# slot arrays
# ---------------------------------------------------------------------------------------------

def slot_mac(fam: str, slot: int) -> bytes:
    """A MAC that names (family, slot): two entries of one address answer differently."""
    return bytes([0x02, ord(fam[0]), (slot >> 16) & 0xFF, (slot >> 8) & 0xFF, slot & 0xFF,
                  0xA4 if fam == "arp" else 0x6D])


def put(table: np.ndarray, slot: int, key, mac=None, valid: bool = True) -> None:
    """An entry written straight into a slot, wherever a probe would have put it."""
    fam = family(table)
    if fam == "arp":
        table["ip"][slot] = key
    else:
        table["ip"][slot] = np.frombuffer(key, np.uint8)
    table["mac"][slot] = np.frombuffer(slot_mac(fam, slot) if mac is None else bytes(mac), np.uint8)
    table["valid"][slot] = 1 if valid else 0


def key_at(table: np.ndarray, slot: int):
    return int(table["ip"][slot]) if family(table) == "arp" else table["ip"][slot].tobytes()


def insert(table: np.ndarray, key) -> int:
    """arp_update / ndp_update (src/arp_table.c:26-53, src/ndp_table.c:39-65): the first slot from
    the home slot that is invalid or holds the address.  Returns the slot."""
    fam, cap = family(table), len(table)
    valid = table["valid"]
    h = home(fam, key, cap)
    for i in range(cap):
        s = (h + i) & (cap - 1)
        if not valid[s] or key_at(table, s) == key:
            put(table, s, key)
            return s
    raise ValueError("table full")


class Probe:
    """The reference's lookup over a slot array: from the home slot, linearly, the first valid
    entry of the address, nothing past the first invalid slot."""

    def __init__(self, table: np.ndarray):
        self.fam, self.cap = family(table), len(table)
        self.valid = table["valid"].astype(bool).tolist()
        self.keys = [key_at(table, s) for s in range(self.cap)]
        self.macs = [table["mac"][s].tobytes() for s in range(self.cap)]

    def slot(self, key) -> int:
        """The slot that answers, or -1."""
        if self.cap == 0:
            return -1
        h = home(self.fam, key, self.cap)
        for i in range(self.cap):
            s = (h + i) & (self.cap - 1)
            if not self.valid[s]:
                return -1
            if self.keys[s] == key:
                return s
        return -1

    def mac(self, key):
        s = self.slot(key)
        return None if s < 0 else self.macs[s]


def stored(table: np.ndarray) -> list:
    """Every address the array holds anywhere (invalid slots' too), in slot order, once each; an
    all-zero address only where its slot is valid."""
    fam, seen, out = family(table), set(), []
    for s in range(len(table)):
        k = key_at(table, s)
        if (k != ZERO[fam] or table["valid"][s]) and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def anatomy(table: np.ndarray) -> dict:
    """What the array holds, by the reference's probe: `reachable` addresses (and the slot that
    answers each), `hidden` ones (in a valid slot, yet no probe finds them), `stale` ones (in
    invalid slots only), `dup` ones (reachable, and in a second valid slot as well)."""
    p = Probe(table)
    out = {"reachable": {}, "hidden": [], "stale": [], "dup": []}
    valid_keys = {}
    for s in range(p.cap):
        if p.valid[s]:
            valid_keys.setdefault(p.keys[s], []).append(s)
    for k in stored(table):
        if k not in valid_keys:
            out["stale"].append(k)
            continue
        s = p.slot(k)
        if s < 0:
            out["hidden"].append(k)
        else:
            out["reachable"][k] = s
            if len(valid_keys[k]) > 1:
                out["dup"].append(k)
    return out


# ---------------------------------------------------------------------------------------------
# the tables, one family at a time
# ---------------------------------------------------------------------------------------------

def _cap1_full(fam):
    t = new_table(fam, 1)
    put(t, 0, homed(fam, 1, 0, 5))
    return t


def _full(fam, cap):
    """Every slot valid: a probe of an absent address ends only after a whole turn.  1024 reachable
    entries take 2048 index slots, the largest staged size."""
    t = new_table(fam, cap)
    for j in range(cap):
        h = j % 3 if cap == 8 else (j * 5) % cap if j % 4 else j % 64
        insert(t, homed(fam, cap, h, j))
    assert t["valid"].all()
    return t


def _wrap(fam):
    t = new_table(fam, 16)
    for j in range(4):
        insert(t, homed(fam, 16, 14, j))   # slots 14, 15, 0, 1
    assert t["valid"][1] and not t["valid"][2], "the chain does not wrap"
    return t


def _hidden(fam):
    """Slot 2 valid, slot 3 invalid, an address of home 2 at slot 4: no probe reaches it."""
    t = new_table(fam, 16)
    put(t, 2, homed(fam, 16, 2, 1))
    put(t, 3, homed(fam, 16, 2, 2), valid=False)
    put(t, 4, homed(fam, 16, 2, 3))
    return t


def _stale_head(fam):
    """What arp_expire leaves at the head of a chain: slot 2 invalid with its address and MAC
    still there; slots 3 and 4 hold addresses of home 3."""
    t = new_table(fam, 16)
    put(t, 2, homed(fam, 16, 2, 1), valid=False)
    put(t, 3, homed(fam, 16, 3, 2))
    put(t, 4, homed(fam, 16, 3, 3))
    return t


def _dup(fam):
    """One address in slots 3 and 4 of a chain, with different MACs: slot 3 answers.  Another in
    slots 15 and 0 of a chain that wraps: slot 15 answers, the copy a walk over the array meets
    second (an index built in slot order from every valid slot would answer with slot 0's)."""
    t = new_table(fam, 16)
    put(t, 2, homed(fam, 16, 2, 1))
    put(t, 3, homed(fam, 16, 2, 2))
    put(t, 4, homed(fam, 16, 2, 2))
    put(t, 5, homed(fam, 16, 2, 3))
    put(t, 14, homed(fam, 16, 14, 4))
    put(t, 15, homed(fam, 16, 14, 5))
    put(t, 0, homed(fam, 16, 14, 5))
    put(t, 1, homed(fam, 16, 14, 6))
    return t


def _key0(fam, with_zero=True):
    """0.0.0.0 / :: inside a chain that wraps: homes 15, 15, 0 (the zero address), 0."""
    t = new_table(fam, 16)
    insert(t, homed(fam, 16, 15, 1))
    insert(t, homed(fam, 16, 15, 2))
    if with_zero:
        assert insert(t, ZERO[fam]) == 1
    insert(t, homed(fam, 16, 0, 3))
    return t


def _combo(fam):
    """Several of the above in one table of 32 slots: a chain that wraps (slots 30 to 2) with an
    address in two of its slots (31 answers, 0 does not) and the zero address in it, a hidden entry
    behind a stale slot, a duplicated address."""
    t = new_table(fam, 32)
    put(t, 30, homed(fam, 32, 30, 0))
    put(t, 31, homed(fam, 32, 30, 1))
    put(t, 0, homed(fam, 32, 30, 1))
    put(t, 1, ZERO[fam])
    put(t, 2, homed(fam, 32, 30, 2))
    put(t, 5, homed(fam, 32, 5, 10))
    put(t, 6, homed(fam, 32, 5, 11), valid=False)
    put(t, 7, homed(fam, 32, 5, 12))
    put(t, 10, homed(fam, 32, 10, 20))
    put(t, 11, homed(fam, 32, 10, 21))
    put(t, 12, homed(fam, 32, 10, 21))
    put(t, 13, homed(fam, 32, 10, 22))
    return t


def one_fold_keys(count: int) -> list:
    """`count` NDP addresses of one fold_v6 (they share all three candidate slots of the index, so
    three can be placed and four cannot), each with a home slot that a 16-slot table and every
    larger one agree on (_ext)."""
    homes = {_ext(16, h) for h in range(16)}
    a = homed("ndp", 16, 3, 77)
    out, aw, j = [a], words("ndp", a), 0
    while len(out) < count:
        j += 1
        b = same_fold(a, aw[1] + j, aw[2] ^ (j << 8), aw[3] + 7 * j)
        bw = words("ndp", b)
        if (bw[0] ^ bw[1] ^ bw[2] ^ bw[3]) & 0xFFFF in homes and b not in out:
            out.append(b)
    assert len({fold_v6(words("ndp", k)) for k in out}) == 1 and len(set(out)) == count
    return out


def _one_fold(fam, count=3):
    t = new_table("ndp", 16)
    for k in one_fold_keys(count):
        insert(t, k)
    return t


def _one_home(fam):
    """Five addresses of home slot 2: four rotations of one set of four words and a swap of
    neighbouring words (equal XOR, so one chain)."""
    w = (0x20010DB8, 0x00000001, 0xA5A50000, 0x00C30DBB)
    t = new_table("ndp", 16)
    for r in range(4):
        insert(t, from_words("ndp", [w[(r + j) % 4] for j in range(4)]))
    insert(t, from_words("ndp", (w[1], w[0], w[3], w[2])))
    assert t["valid"][2:7].all() and t["valid"].sum() == 5
    return t


def _random_key(fam, rng):
    w = [int(x) for x in rng.integers(0, 1 << 32, size=4)]
    return from_words(fam, w if fam == "ndp" else [w[0] | 1 << 31, 0, 0, 0])


def _big4096(fam, seed=4096):
    """4096 slots at about 0.7, as tools/neigh_san.cpp builds its large case: inserted as the
    reference inserts, half the addresses within 2048 homes (chains grow long and merge), one slot
    in 16 knocked out (entries behind the holes become unreachable), 60 addresses inserted again
    (the copy in the hole shadows the one behind it).  Its index passes 2048 slots."""
    rng = np.random.default_rng(seed + (fam == "ndp"))
    t = new_table(fam, 4096)
    keys = []
    for j in range(3000):
        w = list(words(fam, _random_key(fam, rng)))
        if j % 2:
            r = int(rng.integers(0, 2048))
            w[0] = (w[0] & ~0xFFF) | ((w[1] ^ w[2] ^ w[3] ^ r) & 0xFFF)
        k = from_words(fam, w)
        keys.append(k)
        insert(t, k)
    t["valid"][(rng.integers(0, 16, size=4096) == 0) & (t["valid"] == 1)] = 0
    for j in rng.integers(0, len(keys), size=60):
        insert(t, keys[int(j)])
    assert 2700 <= int(t["valid"].sum()) <= 3000
    return t


def _boundary(fam, n, seed=1638):
    """`n` addresses inserted into 4096 slots and nothing else: exactly n reachable entries."""
    rng = np.random.default_rng(seed + (fam == "ndp"))
    t = new_table(fam, 4096)
    while int(t["valid"].sum()) < n:
        insert(t, _random_key(fam, rng))
    return t


_FILLERS: dict = {}


def fillers(fam) -> np.ndarray:
    """FILLERS ordinary entries in BIG slots whose chains stay clear of the first and last CLEAR
    slots (asserted)."""
    if fam not in _FILLERS:
        rng = np.random.default_rng(1700 + (fam == "ndp"))
        t = new_table(fam, BIG)
        while int(t["valid"].sum()) < FILLERS:
            k = _random_key(fam, rng)
            if 4 * CLEAR <= home(fam, k, BIG) < BIG - 4 * CLEAR:
                insert(t, k)
        assert not t["valid"][:CLEAR].any() and not t["valid"][-CLEAR:].any()
        _FILLERS[fam] = t
    return _FILLERS[fam]


def embed_slot(cap: int, s: int) -> int:
    """Where slot s of a `cap`-slot table lies in the embedding table: the lower half at the
    start, the upper half at the end, so that a chain that wraps still wraps."""
    return s if s < cap // 2 else BIG - cap + s


def embed(small: np.ndarray) -> np.ndarray:
    """The table's slots, unchanged, in a table of BIG slots beside FILLERS ordinary entries: the
    same structure behind an index of 4096 slots, which the kernels read from memory
    (neigh_lookup), not from LDS.  Every valid entry's home slot moves with its slot (homed), no
    chain runs across the middle of the small table, and the fillers' chains end CLEAR slots
    away, so every probe walks the slots it walked in the small table."""
    fam, cap = family(small), len(small)
    assert 0 < cap and cap // 2 < CLEAR
    big = fillers(fam).copy()
    if cap > 1:
        assert not (small["valid"][cap // 2 - 1] and small["valid"][cap // 2])
    raw_big = big.view(np.uint8).reshape(BIG, -1)      # whole slots, padding and all
    raw_small = small.view(np.uint8).reshape(cap, -1)
    for s in range(cap):
        raw_big[embed_slot(cap, s)] = raw_small[s]
        if small["valid"][s]:
            k = key_at(small, s)
            assert home(fam, k, BIG) == embed_slot(cap, home(fam, k, cap)), (fam, s)
    lo, hi = big["valid"][:CLEAR].copy(), big["valid"][-CLEAR:].copy()
    lo[:(cap + 1) // 2 if cap > 1 else 0] = 0
    hi[CLEAR - (cap - cap // 2):] = 0
    assert not lo.any() and not hi.any()
    return big


FAMILY_TABLES = {
    "cap0": lambda f: new_table(f, 0),
    "cap1_empty": lambda f: new_table(f, 1),
    "cap1_full": _cap1_full,
    "full8": lambda f: _full(f, 8),
    "full1024": lambda f: _full(f, 1024),
    "wrap": _wrap,
    "hidden": _hidden,
    "stale_head": _stale_head,
    "dup": _dup,
    "key0": _key0,
    "no_key0": lambda f: _key0(f, False),
    "combo": _combo,
    "one_fold": _one_fold,
    "one_home": _one_home,
    "big4096": _big4096,
    "boundary_n": lambda f: _boundary(f, BOUNDARY_N),
    "boundary_n1": lambda f: _boundary(f, BOUNDARY_N + 1),
}
SMALL = ("cap0", "cap1_empty", "cap1_full", "full8", "full1024", "wrap", "hidden", "stale_head",
         "dup", "key0", "no_key0", "combo", "one_fold", "one_home")
# the structural cases that embed() takes (a full table's property is the whole table's)
EMBEDDED = ("cap1_full", "wrap", "hidden", "stale_head", "dup", "key0", "no_key0", "combo",
            "one_fold", "one_home")
_TABLES: dict = {}


def table(fam: str, name: str) -> np.ndarray:
    """Family `fam`'s table of a case, built once; "embed:<name>" is embed() of it.  An NDP-only
    case's ARP table is the duplicated-address one."""
    if fam == "arp" and name.split(":")[-1] in NDP_ONLY:
        name = name.replace(name.split(":")[-1], "dup")
    if (fam, name) not in _TABLES:
        if name.startswith("embed:"):
            t = embed(table(fam, name[6:]))
        else:
            t = FAMILY_TABLES[name](fam)
        t.setflags(write=False)
        _TABLES[fam, name] = t
    return _TABLES[fam, name]


@dataclasses.dataclass
class Case:
    name: str
    arp_name: str
    ndp_name: str

    @property
    def arp(self) -> np.ndarray:
        return table("arp", self.arp_name)

    @property
    def ndp(self) -> np.ndarray:
        return table("ndp", self.ndp_name)

    def table(self, fam: str) -> np.ndarray:
        return self.arp if fam == "arp" else self.ndp

    def own(self, fam: str) -> list:
        """The addresses the batch must reach: an embedded table's are the small table's."""
        name = self.arp_name if fam == "arp" else self.ndp_name
        own = stored(table(fam, name[6:] if name.startswith("embed:") else name))
        return own if len(own) <= 64 else []   # (a large table is all its own: none comes first)


def case(name: str) -> Case:
    """"<t>": both families' table t.  "embed:<t>": both embedded (both indexes in memory).
    "arp-mem:<t>" / "ndp-mem:<t>": that family's index in memory, the other's staged — for an
    embeddable t the embedded table beside the small one, for big4096 beside full1024.
    "boundary:<fam>:<n|n1>": that family's boundary table beside the other's duplicated-address
    one."""
    if name.startswith("boundary:"):
        _, fam, which = name.split(":")
        t = "boundary_" + which
        return Case(name, t if fam == "arp" else "dup", t if fam == "ndp" else "dup")
    if name.startswith(("arp-mem:", "ndp-mem:")):
        fam, t = name[:3], name[8:]
        big, small = (t, "full1024") if t == "big4096" else ("embed:" + t, t)
        return Case(name, big if fam == "arp" else small, big if fam == "ndp" else small)
    return Case(name, name, name)


SMALL_CASES = list(SMALL)
MEMORY_CASES = ["embed:" + t for t in EMBEDDED] + ["big4096"]
BOUNDARY_CASES = [f"boundary:{f}:{w}" for f in ("arp", "ndp") for w in ("n", "n1")]
SPLIT_CASES = [f"{f}-mem:{t}" for t in EMBEDDED + ("big4096",) for f in ("arp", "ndp")]


# ---------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------

def rules(total: int = 8, seed: int = 7) -> np.ndarray:
    """Two DROP rules on ports, a rule with an unknown action, then `total` - 5 fill rules that
    match none of the traffic (exact 5-tuples from 198.18.0.0/15 and 2001:db8::/32, where no
    packet comes from), then one family-wide FWD rule per family: every packet that names none of
    the three ports is forwarded after a walk past the whole table."""
    rng = np.random.default_rng(seed)
    head = synth.rules_array([synth.make_rule(10, ACT_DROP, dport=PORT_DROP_D),
                              synth.make_rule(20, ACT_DROP, sport=PORT_DROP_S),
                              synth.make_rule(30, 2, dport=PORT_ACTION)])
    tail = synth.rules_array([synth.make_rule(1 << 29, ACT_FWD, ip_ver=4),
                              synth.make_rule((1 << 29) + 1, ACT_FWD, ip_ver=6)])
    k = total - 5
    f = np.zeros(k, RULE_DTYPE)
    f["priority"] = 100 + rng.permutation(k)
    v6 = rng.random(k) < 0.4
    f["ip_ver"] = np.where(v6, 6, 4)
    f["protocol"] = rng.choice([6, 17], size=k)
    f["src_port"] = rng.integers(1, 65536, size=k)
    f["dst_port"] = rng.integers(1, 65536, size=k)
    f["action"] = rng.integers(0, 2, size=k)
    f["out_ifindex"] = f["action"]
    for a, m in (("src_ip", "src_mask"), ("dst_ip", "dst_mask")):
        v4 = (0xC6120000 + rng.integers(0, 1 << 17, size=k)).astype("<u4")
        f[a][:, :4] = v4.view(np.uint8).reshape(-1, 4)
        f[m][:, :4] = 0xFF
        a6 = rng.integers(0, 256, size=(k, 16), dtype=np.uint8)
        a6[:, :4] = np.frombuffer(bytes.fromhex("20010db8"), np.uint8)
        f[a][v6] = a6[v6]
        f[m][v6] = 0xFF
    return np.concatenate([head, f, tail])


# ---------------------------------------------------------------------------------------------
# traffic
# ---------------------------------------------------------------------------------------------

def _flip(fam, key, rng):
    w = list(words(fam, key))
    j = int(rng.integers(0, 4)) if fam == "ndp" else 0
    w[j] ^= 1 << int(rng.integers(0, 32))
    return from_words(fam, w)


def _destinations(cs: Case, fam: str, m: int, rng):
    """m destinations of one family, in order, and which of them must be forwarded (the one sure
    packet to each of the case's own addresses).  Once each: every address stored anywhere in the
    slot array (of a table past the batch's size: the case's own and a seeded sample of the rest),
    stored ones with one bit flipped (same chain, or the next), random absent ones, the zero
    address.  The rest of the batch: runs of one destination (L1 hits after the first) and
    alternations of two (every packet past the L1 entry)."""
    t = cs.table(fam)
    all_stored = stored(t)
    own = cs.own(fam)
    room = int(0.45 * m)
    if len(all_stored) > room:
        rest = [k for k in all_stored if k not in set(own)]
        pick = rng.permutation(len(rest))[:room - len(own)]
        base = own + [rest[int(j)] for j in pick]
    else:
        base = list(all_stored)
    held = set(all_stored)
    once = list(base)
    src = own + base if base else []
    nflip = 0 if not src else int(0.2 * m) if len(all_stored) > 64 else max(24, 4 * len(src))
    while nflip > 0:
        k = _flip(fam, src[int(rng.integers(0, len(src)))], rng)
        if k not in held:
            once.append(k)
            nflip -= 1
    once += [_random_key(fam, rng) for _ in range(max(16, m // 10))]
    once += [ZERO[fam]] * 12
    mine = set(own)
    segs = [[(k, j < len(base) and k in mine)] for j, k in enumerate(once)]
    total = len(once)
    # (the case's own addresses lead the runs four times as often as any other)
    lead = own * 4 + once
    while total < m:
        a = lead[int(rng.integers(0, len(lead)))]
        if rng.random() < 0.3:
            b = lead[int(rng.integers(0, len(lead)))]
            seg = [(a, False), (b, False)] * int(rng.integers(1, 4))
        else:
            seg = [(a, False)] * int(rng.integers(2, 7))
        seg = seg[:m - total]
        segs.append(seg)
        total += len(seg)
    order = rng.permutation(len(segs))
    flat = [x for j in order for x in segs[int(j)]]
    return [k for k, _ in flat], np.array([f for _, f in flat], bool)


def traffic(cs: Case, n: int = N_PACKETS, n_rules: int = 8, seed: int = 0) -> synth.Workload:
    """A batch over the case's tables.  Both families alternate packet by packet, then
    keyframes.arrange_runs moves the first quarter of each family into whole 64-packet runs of
    its own and leaves the rest mixed, so that waves of one family and waves of both look up.
    The first IPv6 packet goes to :: (the calloc'd L1 entry answers it) and the last packet of
    the batch to 0.0.0.0; TTL / hop limit 0 or 1 on one packet in 32; six frames do not parse;
    `rules(n_rules)`."""
    rng = np.random.default_rng([seed, n_rules] + list(cs.name.encode()))
    n4 = (n + 1) // 2
    n6 = n - n4
    d4, must4 = _destinations(cs, "arp", n4, rng)
    d6, must6 = _destinations(cs, "ndp", n6, rng)
    d4[-1] = 0
    d6[0] = ZERO["ndp"]
    keys = np.zeros(n, FLOW_KEY_DTYPE)
    is6 = np.arange(n) % 2 == 1
    keys["ip_ver"] = np.where(is6, 6, 4)
    src = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    src[~is6, 3] = 10                       # 10.0.0.0/8 (host order, LE bytes)
    src[is6, 0] = 0xFD                      # fd00::/8
    keys["src_ip"] = src
    dst = np.zeros((n, 16), np.uint8)
    dst[~is6, :4] = np.array(d4, "<u4").view(np.uint8).reshape(-1, 4)
    dst[is6] = np.frombuffer(b"".join(d6), np.uint8).reshape(-1, 16)
    keys["dst_ip"] = dst
    keys["protocol"] = rng.choice([17, 6, 1], size=n, p=[0.6, 0.3, 0.1])
    sport = rng.integers(1024, 60000, size=n)
    dport = rng.integers(1024, 7000, size=n)
    u = rng.random(n)
    dport = np.where(u < 0.05, PORT_DROP_D, np.where(u < 0.08, PORT_ACTION, dport))
    sport = np.where((u >= 0.08) & (u < 0.11), PORT_DROP_S, sport)
    # forwarded for sure (plain ports, and below a TTL above 1): the one packet to each of the
    # case's own addresses, the first IPv6 packet and the last packet
    plain = np.zeros(n, bool)
    plain[~is6], plain[is6] = must4, must6
    plain[[1, n - 1]] = True
    sport[plain], dport[plain] = 2000, 3000
    keys["src_port"], keys["dst_port"] = sport, dport
    keys["protocol"][plain] = 17
    keys = arrange_runs(canonical(keys))
    first6 = int(np.nonzero(keys["ip_ver"] == 6)[0][0])
    assert keys["dst_ip"][first6].tobytes() == bytes(16) and not keys["dst_ip"][n - 1, :4].any()
    frames, desc = frames_from_keys(keys, rng)
    offs, lens = desc_offsets(desc), desc_lens(desc).copy()
    free = np.nonzero((keys["src_port"] != 2000) | (keys["dst_port"] != 3000))[0]
    low = rng.choice(free, size=n // 32 + 6, replace=False)
    broken, low = low[:6], low[6:]
    for i in low:
        o, v4 = int(offs[i]), keys["ip_ver"][i] == 4
        frames[o + (22 if v4 else 21)] = int(rng.integers(0, 2))
        if v4:   # keep the header checksum right
            ihl = int(frames[o + 14] & 0xF)
            frames[o + 24:o + 26] = 0
            h = frames[o + 14:o + 14 + 4 * ihl].astype(np.uint32)
            s = int(((h[0::2] << 8) | h[1::2]).sum())
            while s >> 16:
                s = (s & 0xFFFF) + (s >> 16)
            frames[o + 24], frames[o + 25] = (~s >> 8) & 0xFF, ~s & 0xFF
    for j, i in enumerate(broken):
        if j % 2:
            lens[i] = 20                       # cut inside the IP header
        else:
            frames[int(offs[i]) + 12:int(offs[i]) + 14] = (0x88, 0xB5)   # an unknown ethertype
    desc = make_desc(offs, lens)
    cap = 1024
    while cap < n_rules:
        cap *= 2
    return synth.Workload(cs.name, frames, desc, rules(n_rules), cap, cs.arp.copy(), cs.ndp.copy())


def destinations(wl: synth.Workload):
    """(family 4 / 6 / 0, destination address) per packet, read from the frames' own bytes."""
    offs = desc_offsets(wl.desc)
    fams, dsts = np.zeros(wl.n, np.int64), []
    for i, o in enumerate(offs.tolist()):
        et = (int(wl.frames[o + 12]) << 8) | int(wl.frames[o + 13])
        if et == 0x0800:
            fams[i] = 4
            dsts.append(int.from_bytes(wl.frames[o + 30:o + 34].tobytes(), "big"))
        elif et == 0x86DD:
            fams[i] = 6
            dsts.append(wl.frames[o + 38:o + 54].tobytes())
        else:
            dsts.append(None)
    return fams, dsts

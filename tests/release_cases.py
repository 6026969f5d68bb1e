"""Classified batches whose forwarded set, replies and bursts are chosen, for the release order
(upe_gpu_release_order, upe_release_order_host, release.order_host, upe_release_flush).

Verdict words are made by hand, which the contract allows: the forwarded set follows
egress_cases' lane patterns put next to each other in every order (64-groups that forward
nothing, everything, only lane 0, only lane 63, lanes 31 and 32, alternate lanes, the two seeded
densities), the other packets cycle through every verdict code that does not forward, and the
reply flag is placed on its own: nowhere, once in every burst, on the first or on the last packet
of every burst, or only on the last packet of the batch — whatever that packet's code is, since
only the flag bit decides.

Bursts: the fixed sizes FIXED, and offset arrays (SHAPES) with lengths cycling 1..64, all ones, 64s
with a short last burst, and 64s shifted so that a burst straddles every multiple of 64 in its
middle (and with it every multiple of 1024), or with one packet on one side of it.

tests/test_release_cases.py pins the host forms on the CPU; tests/test_gpu_release_order.py runs
the same cases on the device.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import egress_cases as ec
from upe_amd.layout import VF_ARP_REPLY

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4 * 1024 + 37)
FIXED = (1, 31, 32, 33, 48, 63, 64)
REPLIES = ("none", "every_burst", "burst_first", "burst_last", "batch_last")
POISON = np.uint32(0xA5A5A5A5)   # no position, count or handle of a case comes near it
ROOM = 16                        # poisoned entries behind every output


def _from_lengths(n: int, lengths) -> np.ndarray:
    first, k = [0], 0
    while first[-1] < n:
        first.append(min(n, first[-1] + int(lengths(k))))
        k += 1
    return np.array(first, np.uint32)


def _shifted(n: int, head: int) -> np.ndarray:
    """A first burst of `head` packets, then 64s: burst k + 1 is [head + 64 k, head + 64 k + 64)."""
    return _from_lengths(n, lambda k: head if k == 0 else 64)


SHAPES = {
    "cycle": lambda n: _from_lengths(n, lambda k: 1 + k % 64),
    "ones": lambda n: np.arange(n + 1, dtype=np.uint32),
    "64s": lambda n: _from_lengths(n, lambda k: 64),
    "straddle_mid": lambda n: _shifted(n, 32),       # 32 packets on each side of a multiple of 64
    "straddle_before": lambda n: _shifted(n, 63),    # one packet before it, 63 from it on
    "straddle_after": lambda n: _shifted(n, 1),      # 63 before it, the multiple itself last
}


def fwd_mask(n: int, shift: int = 0) -> np.ndarray:
    """n lanes of the pair sequence, from its group `shift` on (so that short batches see other
    patterns than the first)."""
    return np.resize(np.roll(ec.pair_mask(), -64 * shift), n)


def words(mask: np.ndarray) -> np.ndarray:
    """Verdict words with the given forwarded set and no reply flag: the kinds' words with rule
    bits that vary, as a classify launch would leave them."""
    v = ec.KIND_VERDICT[ec.kinds_of(mask)] & ~np.uint32(VF_ARP_REPLY)
    return (v | ((1 + np.arange(len(v)) % 7) << 8).astype(np.uint32)).astype(np.uint32)


def with_replies(v: np.ndarray, first: np.ndarray, mode: str) -> np.ndarray:
    f = first.astype(np.int64)
    at = {"none": f[:0], "every_burst": (f[:-1] + f[1:]) // 2, "burst_first": f[:-1],
          "burst_last": f[1:] - 1, "batch_last": f[-1:] - 1}[mode]
    out = v.copy()
    out[at] |= np.uint32(VF_ARP_REPLY)
    return out


@dataclasses.dataclass
class Case:
    name: str
    verdict: np.ndarray
    first: np.ndarray          # the offsets, in either form
    burst: int                 # the fixed size, or 0: the offset array is what the call gets

    @property
    def n(self) -> int:
        return len(self.verdict)

    @property
    def bursts(self) -> list:
        f = self.first.tolist()
        return list(zip(f[:-1], f[1:]))

    @property
    def form(self) -> dict:
        """The burst arguments of release.order_host / gpu.release_order_host."""
        return {"burst": self.burst} if self.burst else {"first": self.first}


def cases(n: int):
    """Every burst shape with every reply placement over n packets."""
    k = 0
    shapes = [(f"fixed{b}", b) for b in FIXED] + [(name, 0) for name in SHAPES]
    for name, b in shapes:
        first = (np.append(np.arange(0, n, b, dtype=np.uint32), np.uint32(n)) if b
                 else SHAPES[name](n))
        assert first[0] == 0 and first[-1] == n and np.all(np.diff(first.astype(np.int64)) >= 1)
        assert np.all(np.diff(first.astype(np.int64)) <= 64)
        for mode in REPLIES:
            v = with_replies(words(fwd_mask(n, k)), first, mode)
            k += 1
            yield Case(f"n{n}:{name}:{mode}", v, first, b)


def slots(n: int, kind: str) -> np.ndarray:
    """Handles: a permutation far from the positions, repeating ones, or descending ones."""
    i = np.arange(n, dtype=np.uint64)
    if kind == "permuted":
        return (100000 + np.random.default_rng([31, n]).permutation(n)).astype(np.uint32)
    if kind == "repeat":
        return (7 + i % 5).astype(np.uint32)
    assert kind == "descend"
    return (3 * n + 11 - 3 * i).astype(np.uint32)


def bad_arrays(n: int) -> dict:
    """name -> (offset array, the violated conditions) for n >= 130 packets in 64s: each breaks
    the rules in one known way."""
    assert n >= 130
    good = SHAPES["64s"](n).astype(np.int64)
    last = int(good[-1] - good[-2])

    def changed(at: int, value: int) -> np.ndarray:
        f = good.copy()
        f[at] = value
        return f

    swapped = good.copy()                         # bursts of 128, -64 and 128 (or n - 64 > 64)
    swapped[1], swapped[2] = good[2], good[1]
    out = {
        "first_not_0": (changed(0, 1), 1),        # the first burst still holds 63
        "last_not_n": (changed(-1, n - 1), 1 if last > 1 else 2),
        "last_past_n": (changed(-1, n + 1), 1 if last < 64 else 2),
        "zero_length": (np.insert(good, 1, good[1]), 1),
        "65_packets": (changed(1, 65), 1),        # 65 packets, then 63
        "descending": (swapped, 3),
    }
    return {k: (a.astype(np.uint32), c) for k, (a, c) in out.items()}

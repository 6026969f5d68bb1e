"""Latency-histogram cases (include/upe_gpu.h "Latency histogram"), each built for one purpose.
Shared by tests/test_latency_cases.py (host: the numpy mirror and the C functions against the
reference's latency_record, or the golden without it), tests/test_gpu_latency.py (the device
against the mirror) and tests/golden/make_latency_golden.py.

A case is (name, timestamps uint64[n], verdicts uint32[n] or None, now, cycles_per_ns,
ref_defined).  ref_defined is False where the reference's cast is undefined behaviour (a quotient
of 2^64 or more): those are compared with the mirror only."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from upe_amd import latency
from upe_amd.layout import (V_CONSUMED, V_DROP_ACTION, V_DROP_NOMATCH, V_DROP_PARSE, V_DROP_RULE,
                            V_DROP_TTL, V_FWD, VF_ARP_LEARN, VF_ARP_REPLY, VF_L1_INIT,
                            VF_NEIGH_HIT)

M64 = 2**64 - 1
CPNS = (2.0, 2.4, 2.3999999, 0.7, 3.3333333333, 1.0, 1.0 / 3.0)
PERCENTILES = (0.0, 0.5, 0.95, 0.99, 0.999, 1.0)
NOW = 0x9E3779B97F4A7C15   # no case's cycle count equals it, so no timestamp comes out as 0


class Case(NamedTuple):
    name: str
    ts: np.ndarray
    verdicts: Optional[np.ndarray]
    now: int
    cpn: float
    ref_defined: bool = True


def from_cycles(name, cycles, cpn, verdicts=None, now=NOW, ref_defined=True) -> Case:
    """Timestamps such that (now - ts) mod 2^64 is each cycle count."""
    cycles = [int(c) & M64 for c in cycles]
    assert now not in cycles
    ts = np.array([(now - c) & M64 for c in cycles], np.uint64)
    v = None if verdicts is None else np.ascontiguousarray(verdicts, np.uint32)
    return Case(name, ts, v, now, float(cpn), ref_defined)


def bound_cycles(cpn: float) -> list:
    """Cycle counts within 3 of where ns crosses each bucket bound."""
    out = []
    for b in latency.BOUNDS:
        c0 = int(b * cpn)
        out += [max(c0 + d, 0) for d in range(-3, 4)]
    return out


def mixed_verdicts(n: int, seed: int) -> np.ndarray:
    """Every verdict code with every flag and a rule index, all seven codes inside each 64-group;
    ARP-flagged DROP_PARSE words among them (ARP leaves through the parse-fail exit and is
    sampled)."""
    rng = np.random.default_rng(seed)
    codes = np.array([V_DROP_PARSE, V_DROP_NOMATCH, V_DROP_RULE, V_DROP_TTL, V_FWD, V_CONSUMED,
                      V_DROP_ACTION], np.uint32)
    flags = np.array([0, VF_NEIGH_HIT, VF_ARP_LEARN, VF_ARP_REPLY, VF_L1_INIT,
                      VF_ARP_LEARN | VF_ARP_REPLY, 0xF0], np.uint32)
    v = np.zeros(n, np.uint32)
    for g in range(0, n, 64):
        m = min(64, n - g)
        c = codes[(np.arange(m) + g // 64) % 7]
        rng.shuffle(c)
        v[g:g + m] = c | flags[rng.integers(0, len(flags), m)] | \
            (rng.integers(0, 1 << 24, m).astype(np.uint32) << np.uint32(8))
    arp = np.nonzero((v & 0xF) == V_DROP_PARSE)[0][::2]
    v[arp] = V_DROP_PARSE | VF_ARP_LEARN
    v[arp[::2]] |= VF_ARP_REPLY   # an answered request
    return v


def random_cycles(n: int, seed: int) -> np.ndarray:
    """Cycle counts whose ns spread over every bucket at the calibrations used here: 2^k scaled,
    k uniform in [0, 40)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 40, n)
    return (rng.integers(0, 1 << 40, n, dtype=np.uint64) >> (40 - k - 1).astype(np.uint64))


def sized(n: int, seed: int = 7, cpn: float = 2.4) -> Case:
    """n packets: random cycle counts over every bucket, the mixed verdict words, and roughly one
    timestamp in eight zero (a buffer nobody stamped)."""
    rng = np.random.default_rng(seed + 31 * n)
    c = from_cycles(f"sized_{n}", random_cycles(n, seed + n).tolist(), cpn,
                    mixed_verdicts(n, seed + 2 * n))
    ts = c.ts.copy()
    ts[rng.integers(0, 8, n) == 0] = 0
    return c._replace(ts=ts)


def cases() -> list:
    out = []
    # every bucket bound +-3 cycles, per calibration
    for cpn in CPNS:
        out.append(from_cycles(f"bounds_cpn_{cpn!r}", bound_cycles(cpn), cpn))
    # 2000 random 40-bit cycle counts per calibration of the issue's list
    rng = np.random.default_rng(11)
    for cpn in CPNS[:6]:
        out.append(from_cycles(f"random40_cpn_{cpn!r}",
                               rng.integers(1, 1 << 40, 2000, dtype=np.uint64).tolist(), cpn))
    # above 2^53 the conversion to double rounds (to nearest even): odd counts, ties, both ways
    big = [2**53 + 1, 2**53 + 2, 2**53 + 3, 2**54 + 2, 2**54 + 6, 2**60 + 129, 2**62 + 12345,
           2**63 - 1, 2**63 - 513, 2**63 - 511]
    out.append(from_cycles("above_2_53_cpn_1", big, 1.0))
    out.append(from_cycles("above_2_53_cpn_2.4", big + [2**63 + 1025, 2**64 - 1], 2.4))
    out.append(from_cycles("above_2_53_cpn_2", big + [2**63 + 1025, 2**64 - 1, 2**64 - 1025], 2.0))
    # timestamps later than `now`: the subtraction wraps, ns is about 2^63 at 2 cycles per ns, and
    # two such samples wrap sum_ns
    now = 123456789
    out.append(Case("wrapped_subtraction", np.array([now + 1, now + 2, now + 1000003, now - 700],
                                                    np.uint64), None, now, 2.0))
    # nothing sampled: count 0, min 1000000, max 0
    out.append(Case("all_timestamps_zero", np.zeros(300, np.uint64),
                    mixed_verdicts(300, 1), NOW, 2.4))
    c = sized(300, 3)
    out.append(c._replace(name="all_consumed",
                          verdicts=(c.verdicts & ~np.uint32(0xF)) | np.uint32(V_CONSUMED)))
    # every code and flag per 64-group
    out.append(sized(1000, 5)._replace(name="mixed_verdicts"))
    out.append(sized(1000, 5)._replace(name="no_verdicts", verdicts=None))
    # every sample in one bucket: all the atomic traffic on one word
    rng = np.random.default_rng(13)
    out.append(from_cycles("one_bucket", (rng.integers(100, 500, 1500) * 2).tolist(), 2.0))
    # every sample above 1 ms: min_ns stays 1000000
    out.append(from_cycles("all_above_1ms", (rng.integers(10**6, 10**9, 700) * 2).tolist(), 2.0))
    out.append(from_cycles("single", [4242], 2.4))
    out.append(from_cycles("single_zero_cycles", [0], 2.4, now=0x8000000000000000))
    # where the reference's cast is undefined: quotients of 2^64 or more saturate
    out.append(from_cycles("saturate_cpn_1", [2**64 - 1, 2**64 - 1024, 2**64 - 1025, 77], 1.0,
                           ref_defined=False))
    out.append(from_cycles("saturate_cpn_half", [2**63, 2**63 - 512, 2**63 - 513, 2**64 - 1, 5],
                           0.5, ref_defined=False))
    out.append(from_cycles("saturate_cpn_tiny", [1, 2, 2**40], 1e-300, ref_defined=False))
    out.append(from_cycles("saturate_cpn_subnormal", [1, 0], 5e-324, now=0x8000000000000000,
                           ref_defined=False))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def expected(c: Case, start=None) -> np.ndarray:
    """The mirror's histogram after the case, from `start` (default: the init state)."""
    return latency.record_host(latency.init() if start is None else start, c.ts, c.verdicts,
                               c.now, c.cpn)

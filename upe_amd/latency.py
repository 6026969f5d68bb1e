"""The worker's latency histogram on the host, in numpy and Python integers: the rules of
include/upe_gpu.h "Latency histogram" (reference include/latency.h:21-40, src/latency.c:35-90,
and the sampling condition of src/worker.c:120-122 ... 249-251), against which
upe_latency_record_batch and upe_gpu_latency_record are checked.

A histogram is 12 uint64 words, the layout of upe_latency_hist_t: buckets[8], total_count, min_ns,
max_ns, sum_ns.  Exact for every cycle count up to 2^64 - 1: the conversion to double goes through
the two 32-bit halves (each exact, one rounding in the sum), the division is numpy's IEEE double
division, and the conversion back is only ever asked of values below 2^64 (a quotient at or above
that saturates, as the header says; numpy's out-of-range cast is not relied on)."""
from __future__ import annotations

import math

import numpy as np

from .layout import V_CONSUMED

BUCKETS = 8                                                  # UPE_LATENCY_BUCKETS
BOUNDS = (100, 500, 1000, 5000, 10000, 50000, 100000, 1000000)   # UPE_LATENCY_BOUNDS
MIN_INIT = 1000000                                           # UPE_LATENCY_MIN_INIT
WORDS = BUCKETS + 4
TOTAL, MIN, MAX, SUM = 8, 9, 10, 11                          # word indexes after the buckets
U64_MAX = 2**64 - 1
_TWO64 = 18446744073709551616.0


def init() -> np.ndarray:
    """upe_latency_init."""
    h = np.zeros(WORDS, np.uint64)
    h[MIN] = MIN_INIT
    return h


def cpn_ok(cycles_per_ns) -> bool:
    """A calibration the library accepts: finite and > 0."""
    x = float(cycles_per_ns)
    return math.isfinite(x) and x > 0.0


def to_ns(cycles: np.ndarray, cycles_per_ns: float) -> np.ndarray:
    """ns of each cycle count (uint64 in, uint64 out), saturating at 2^64 - 1."""
    c = np.ascontiguousarray(cycles, np.uint64)
    hi = (c >> np.uint64(32)).astype(np.float64)
    lo = (c & np.uint64(0xFFFFFFFF)).astype(np.float64)
    with np.errstate(over="ignore"):
        q = (hi * 4294967296.0 + lo) / np.float64(cycles_per_ns)
    over = ~(q < _TWO64)
    ns = np.where(over, 0.0, q).astype(np.uint64)   # in range: truncates
    ns[over] = np.uint64(U64_MAX)
    return ns


def sampled(timestamps: np.ndarray, verdicts=None) -> np.ndarray:
    """Which packets are sampled: a non-zero timestamp and a verdict code other than CONSUMED."""
    take = np.ascontiguousarray(timestamps, np.uint64) != 0
    if verdicts is not None:
        take &= (np.asarray(verdicts, np.uint32) & np.uint32(0xF)) != V_CONSUMED
    return take


def record_host(hist: np.ndarray, timestamps, verdicts, now: int, cycles_per_ns: float) -> np.ndarray:
    """upe_latency_record_batch: the histogram after the batch (a new array; `hist` is not
    written).  Raises ValueError for a calibration the library refuses."""
    if not cpn_ok(cycles_per_ns):
        raise ValueError("cycles_per_ns must be finite and > 0")
    ts = np.ascontiguousarray(timestamps, np.uint64)
    take = sampled(ts, verdicts)
    with np.errstate(over="ignore"):
        cycles = np.uint64(now & U64_MAX) - ts[take]      # wraps modulo 2^64
    ns = to_ns(cycles, cycles_per_ns)
    out = np.array(hist, np.uint64).copy()
    if ns.size == 0:
        return out
    bucket = np.minimum(np.searchsorted(np.array(BOUNDS, np.uint64), ns, side="right"), BUCKETS - 1)
    h = [int(x) for x in out]
    for b, k in zip(*np.unique(bucket, return_counts=True)):
        h[int(b)] = (h[int(b)] + int(k)) & U64_MAX
    h[TOTAL] = (h[TOTAL] + int(ns.size)) & U64_MAX
    h[SUM] = (h[SUM] + sum(ns.tolist())) & U64_MAX
    h[MIN] = min(h[MIN], int(ns.min()))
    h[MAX] = max(h[MAX], int(ns.max()))
    return np.array(h, np.uint64)


def percentile(hist: np.ndarray, p: float) -> int:
    """upe_latency_percentile."""
    total = int(hist[TOTAL])
    if total == 0:
        return 0
    want = float(p) * float(total)
    target = 0 if not want > 0.0 else U64_MAX if want >= _TWO64 else int(want)
    cumulative = 0
    for i in range(BUCKETS):
        cumulative = (cumulative + int(hist[i])) & U64_MAX
        if cumulative >= target:
            return BOUNDS[i]
    return BOUNDS[-1]


def merge(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """upe_latency_merge: dst after src is merged into it (a new array)."""
    d, s = [int(x) for x in dst], [int(x) for x in src]
    out = [(a + b) & U64_MAX for a, b in zip(d[:BUCKETS], s[:BUCKETS])]
    out += [(d[TOTAL] + s[TOTAL]) & U64_MAX, min(d[MIN], s[MIN]), max(d[MAX], s[MAX]),
            (d[SUM] + s[SUM]) & U64_MAX]
    return np.array(out, np.uint64)

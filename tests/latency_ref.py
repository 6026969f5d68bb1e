"""Expected latency histograms from the reference itself: its latency_record called once per
sampled packet (oracle/_ref/libupe_ref.so links the reference's src/latency.c), and the golden
file that records those results for machines without the reference
(tests/golden/latency_cases.npz, written by tests/golden/make_latency_golden.py)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

import latency_cases
import oracle
from upe_amd import latency

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_cases.npz")
_M64 = 2**64 - 1
_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        x = oracle.ref_lib()
        P = ctypes.c_void_p
        x.latency_histogram_init.restype = None
        x.latency_histogram_init.argtypes = [P]
        x.latency_record.restype = None
        x.latency_record.argtypes = [P, ctypes.c_uint64, ctypes.c_double]
        x.latency_percentile.restype = ctypes.c_uint64
        x.latency_percentile.argtypes = [P, ctypes.c_double]
        x.latency_histogram_merge.restype = None
        x.latency_histogram_merge.argtypes = [P, P]
        _lib = x
    return _lib


def _p(h: np.ndarray):
    assert h.dtype == np.uint64 and h.size == latency.WORDS and h.flags["C_CONTIGUOUS"]
    return h.ctypes.data_as(ctypes.c_void_p)


def ref_init() -> np.ndarray:
    h = np.full(latency.WORDS, 0xA5A5A5A5A5A5A5A5, np.uint64)
    lib().latency_histogram_init(_p(h))
    return h


def ref_record(c: latency_cases.Case, start=None) -> np.ndarray:
    """The reference's histogram after the case's sampled packets, one latency_record each, in
    packet order (only for cases with ref_defined)."""
    assert c.ref_defined
    h = ref_init() if start is None else np.array(start, np.uint64)
    rec, hp = lib().latency_record, _p(h)
    take = latency.sampled(c.ts, c.verdicts)
    for t in c.ts[take].tolist():
        rec(hp, (c.now - t) & _M64, c.cpn)
    return h


def ref_percentiles(h: np.ndarray) -> np.ndarray:
    h = np.ascontiguousarray(h, np.uint64)
    return np.array([lib().latency_percentile(_p(h), p) for p in latency_cases.PERCENTILES],
                    np.uint64)


def ref_merge(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    d, s = np.array(dst, np.uint64), np.ascontiguousarray(src, np.uint64)
    lib().latency_histogram_merge(_p(d), _p(s))
    return d


def build_golden() -> dict:
    """The golden file's arrays, from the reference (needs oracle.ref_available())."""
    out = {}
    names = []
    for c in latency_cases.cases():
        if not c.ref_defined:
            continue
        k = len(names)
        names.append(c.name)
        h = ref_record(c)
        out[f"ts_{k}"] = c.ts
        if c.verdicts is not None:
            out[f"verdicts_{k}"] = c.verdicts
        out[f"now_{k}"] = np.array(c.now, np.uint64)
        out[f"cpn_{k}"] = np.array(c.cpn, np.float64)
        out[f"hist_{k}"] = h
        out[f"pct_{k}"] = ref_percentiles(h)
    out["names"] = np.array(names)
    out["percentiles"] = np.array(latency_cases.PERCENTILES, np.float64)
    return out


def load_golden() -> dict:
    """name -> (Case as stored, the reference's histogram, its percentiles)."""
    z = np.load(GOLDEN)
    out = {}
    for k, name in enumerate(z["names"].tolist()):
        v = z[f"verdicts_{k}"] if f"verdicts_{k}" in z.files else None
        c = latency_cases.Case(name, z[f"ts_{k}"], v, int(z[f"now_{k}"]), float(z[f"cpn_{k}"]))
        out[name] = (c, z[f"hist_{k}"], z[f"pct_{k}"])
    return out

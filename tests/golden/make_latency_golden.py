"""Generate tests/golden/latency_cases.npz from the REFERENCE's own latency_record.

Runs only where oracle/_ref/libupe_ref.so exists (it links the reference's src/latency.c).  The
output is data only: for every case of tests/latency_cases.py that the reference defines, the
inputs (timestamps, verdict words, now, cycles_per_ns) and the reference's results — the 12 words
of its latency_histogram_t after one latency_record per sampled packet, and latency_percentile at
the percentiles of latency_cases.PERCENTILES.

Usage: python tests/golden/make_latency_golden.py   (from the repo root, after `make -C oracle`)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import latency_ref  # noqa: E402
import oracle  # noqa: E402


def main() -> None:
    if not oracle.ref_available():
        raise SystemExit("oracle/_ref/libupe_ref.so is not built: the reference is needed")
    arrays = latency_ref.build_golden()
    np.savez_compressed(latency_ref.GOLDEN, **arrays)
    print(f"{latency_ref.GOLDEN}: {len(arrays['names'])} cases, "
          f"{os.path.getsize(latency_ref.GOLDEN)} bytes")


if __name__ == "__main__":
    main()

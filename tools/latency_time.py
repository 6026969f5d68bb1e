"""Time of upe_gpu_latency_record's launch on GPU 0, beside a plain hipMemcpyAsync (device to
device) of the bytes the call must read, taken on the same stream in the same run.  All in one
process.

  python tools/latency_time.py [--out profiles/latency_record.json] [--n 1048576] [--reps 30]

Rows: n packets with and without verdict words, and n / 16 packets with them (a worker-loop sized
batch).  Timestamps and verdicts are latency_cases-style: cycle counts over every bucket, every
verdict code per 64-group, one timestamp in eight zero.
launch_us: HIP events around the launch (upe_gpu_latency_record_timed), median of --reps calls
after 5 warm-up ones; copy_us: hipMemcpyAsync of must_bytes between two events, the same calls.
call_us: a host clock around --reps back-to-back asynchronous calls ending in a synchronise, per
call (no events between the launches).
must_bytes: what the contract makes the call read, per packet 8 (timestamp) + 4 (verdict word,
when given); it writes at most 12 words per workgroup.
The device result of the timed calls is checked against latency.record_host."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import latency_cases
    from upe_amd import gpu, latency

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latency_record.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    reps = args.reps

    P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    timed = gpu.LIB.upe_gpu_latency_record_timed
    timed.restype = I
    timed.argtypes = [P, P, P, SZ, ctypes.c_uint64, P, P, SZ, P, P]

    rows = []
    for n, with_verdicts in ((args.n, True), (args.n, False), (max(args.n // 16, 1), True)):
        c = latency_cases.sized(n, 23)
        if not with_verdicts:
            c = c._replace(verdicts=None)
        must = n * (12 if with_verdicts else 8)
        w = gpu.GpuWorker(0, 16)
        w.set_tsc(c.cpn)
        d_ts, d_v = w.malloc(8 * n), w.malloc(4 * n) if with_verdicts else 0
        w.h2d(d_ts, c.ts)
        if with_verdicts:
            w.h2d(d_v, c.verdicts)
        d_src, d_dst = w.malloc(must), w.malloc(must)
        w.sync()
        ms = (ctypes.c_float * 2)()
        took = []
        for j in range(5 + reps):
            rc = timed(w._ctx, d_ts, d_v or None, n, c.now, d_src, d_dst, must, None, ms)
            if rc != 0:
                raise RuntimeError(gpu.LIB.upe_gpu_last_error().decode())
            if j >= 5:
                took.append(tuple(ms))
        med = [1e3 * statistics.median(t[j] for t in took) for j in range(2)]
        w.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            w.latency_record(d_ts, d_v or None, n, c.now)
        w.sync()
        whole = 1e6 * (time.perf_counter() - t0) / reps
        # 5 + reps timed calls and reps plain ones of the same batch
        one = latency.record_host(latency.init(), c.ts, c.verdicts, c.now, c.cpn)
        want = latency.init()
        for _ in range(5 + 2 * reps):
            want = latency.merge(want, one)
        got = w.get_latency()
        assert got.tolist() == want.tolist(), (got, want)
        row = {"n": n, "verdicts": with_verdicts, "must_bytes": must,
               "sampled": int(one[latency.TOTAL]),
               "launch_us": round(med[0], 1), "launch_GBps": round(must / med[0] / 1e3, 1),
               "ns_per_packet": round(1e3 * med[0] / n, 4),
               "copy_us": round(med[1], 1), "copy_GBps": round(must / med[1] / 1e3, 1),
               "launch_over_copy": round(med[0] / med[1], 2), "call_us": round(whole, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (d_ts, d_v, d_src, d_dst):
            if p:
                w.free(p)
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/latency_time.py", "device": "MI355X",
                   "block": gpu.LATENCY_BLOCK, "reps": reps, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

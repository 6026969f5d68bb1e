"""Time of upe_gpu_rx_dispatch's three passes (hash, scan, scatter) on GPU 0, beside the plain
classify launch of the same batch and rx.dispatch_host on the host, all in one process.

  python tools/rx_dispatch_time.py [--out profiles/rx_dispatch.json] [--n 1048576] [--reps 50]

Workloads: synth.config_b(n, seed=2) (64-byte UDP, every packet parses) and a config-D draw of
the same size (4096 rules; mixed families, IPv4 options, about 7 % fallback packets), each at 2
and 64 rings.
Per pass: HIP events around each launch (upe_gpu_rx_dispatch_timed), median of --reps dispatches
after 5 warm-up ones.  dispatch_ms: a host clock around --reps back-to-back asynchronous dispatches
ending in a synchronise, per dispatch (no events between the launches).  classify_ms: the
library's own event timing of upe_gpu_process (upe_gpu_timing_*), the frames uploaded again before
every launch since the path rewrites them.  host_ms: rx.dispatch_host over the hashes the device
produced (median of 5).  The device result is checked against rx.dispatch_host before timing."""
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


def main() -> None:
    from upe_amd import gpu, rx, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rx_dispatch.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    n, reps = args.n, args.reps

    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    timed = gpu.LIB.upe_gpu_rx_dispatch_timed
    timed.restype = ctypes.c_int
    timed.argtypes = [P, P, P, ctypes.c_size_t, U32, U32, P, P, P, P, P, P, P]

    rows = []
    for name, make in (("B", lambda: synth.config_b(n=n, seed=2)),
                       ("D", lambda: synth.config_d(n=n, seed=4, n_rules=1 << 12))):
        wl = make()
        w = gpu.GpuWorker(0, wl.capacity)
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        ring, index, fh, dout = (w.malloc(4 * n), w.malloc(4 * n), w.malloc(4 * n),
                                 w.malloc(8 * n))
        frame_bytes = float(np.minimum(wl.desc & np.uint64(0xFFFF), 80).mean())
        for rings in (2, 64):
            counts = w.malloc(8 * (rings + 1))
            w.rx_dispatch(b.frames, b.desc, n, rings, 0, ring, index, counts, flow_hash=fh,
                          desc_out=dout)
            got = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
                   np.zeros(rings + 1, np.uint64)]
            w.sync()
            for host, dev in zip(got, (ring, index, fh, counts)):
                w.d2h(host, dev)
            w.sync()
            ok = (got[0] & np.uint32(rx.FALLBACK)) == 0
            want = rx.dispatch_host(got[2], ok, rings, 0)
            assert all(np.array_equal(x, y) for x, y in zip((got[0], got[1], got[3]), want[:3]))
            ms = (ctypes.c_float * 3)()
            passes = []
            for k in range(5 + reps):
                rc = timed(w._ctx, b.frames, b.desc, n, rings, 0, ring, fh, index, dout, counts,
                           None, ms)
                if rc != 0:
                    raise RuntimeError(gpu.LIB.upe_gpu_last_error().decode())
                if k >= 5:
                    passes.append(tuple(ms))
            med = [statistics.median(p[j] for p in passes) for j in range(3)]
            w.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                w.rx_dispatch(b.frames, b.desc, n, rings, 0, ring, index, counts, flow_hash=fh,
                              desc_out=dout)
            w.sync()
            whole = 1e3 * (time.perf_counter() - t0) / reps
            host = []
            for _ in range(5):
                t0 = time.perf_counter()
                rx.dispatch_host(got[2], ok, rings, 0)
                host.append(1e3 * (time.perf_counter() - t0))
            rows.append({"workload": name, "n": n, "rings": rings,
                         "fallback_packets": int(got[3][rings]),
                         "header_bytes_per_packet": round(frame_bytes, 1),
                         "hash_ms": round(med[0], 4), "scan_ms": round(med[1], 4),
                         "scatter_ms": round(med[2], 4), "passes_ms": round(sum(med), 4),
                         "dispatch_ms": round(whole, 4),
                         "host_ms": round(statistics.median(host), 3)})
            w.free(counts)
        # the plain classify launch of the same batch (it rewrites the frames: upload them again)
        for k in range(3 + min(reps, 20)):
            if k == 3:
                w.sync()
                w.timing_enable(1)
            w.h2d(b.frames, wl.frames)
            b.run()
        c_ms, _, launches = w.timing_read()
        w.timing_enable(0)
        for r in rows:
            if r["workload"] == name:
                r["classify_ms"] = round(c_ms / max(launches, 1), 4)
        for p in (ring, index, fh, dout):
            w.free(p)
        b.free()
        w.close()
        for r in rows:
            if r["workload"] == name:
                print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/rx_dispatch_time.py", "device": "MI355X", "rows": rows}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

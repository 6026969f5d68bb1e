"""Time of upe_gpu_ingress_gather's passes (size and marks, scan, write) on GPU 0 for a burst of
handles in random order over a stride-2064 pktbuf pool, beside a plain hipMemcpyAsync of the bytes
the call must move, taken on the same stream in the same run (device to device for a pool in HBM,
host to device for a pool in pinned host memory).  All in one process.

  python tools/ingress_gather_time.py [--out profiles/ingress_gather.json] [--n 1048576]
                                      [--reps 30]

Workloads: n frames of 64 bytes, and n frames of the IMIX mix (64 / 570 / 1518 bytes, 7 : 4 : 1),
one per buffer, the handles a random permutation of the pool's n buffers.  Rows: REF, WINDOW and
FULL with the pool in HBM, WINDOW and REF with the pool in pinned host memory (the outputs always
in HBM).
Per pass: HIP events around each launch (upe_gpu_ingress_gather_timed), median of --reps calls
after 5 warm-up ones; copy_us: hipMemcpyAsync of must_bytes between two events, the same calls.
call_us: a host clock around --reps back-to-back asynchronous calls ending in a synchronise, per
call (no events between the launches).
must_bytes: what the contract makes the call read and write, per packet 4 (handle) + 16 (buffer
header) + 16 (descriptor and timestamp out) plus REF: the 32 frame bytes the control mark looks
at; WINDOW: the frame's quads inside the window in, 96 out; FULL: the frame's quads in and out.
The device result of the first 65536 handles is checked against ingress.gather_host before
timing."""
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

STRIDE = 2064


def make_pool(n, lens, seed):
    """n buffers, buffer k holding a frame of lens[k] random bytes (timestamp k + 1)."""
    rng = np.random.default_rng(seed)
    pool = np.zeros((n, STRIDE), np.uint8)
    head = np.zeros((n, 2), "<u8")
    head[:, 0] = np.arange(1, n + 1)
    head[:, 1] = lens
    pool[:, :16] = head.view(np.uint8)
    for ln in np.unique(lens):
        rows = np.nonzero(lens == ln)[0]
        pool[rows, 16:16 + ln] = rng.integers(0, 256, (rows.size, int(ln)), dtype=np.uint8)
    return pool.reshape(-1)


def main() -> None:
    from upe_amd import gpu, ingress
    from upe_amd.layout import HDR_WINDOW, INGRESS_INFO_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingress_gather.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    n, reps = args.n, args.reps

    P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    timed = gpu.LIB.upe_gpu_ingress_gather_timed
    timed.restype = I
    timed.argtypes = [P, P, SZ, SZ, P, SZ, I, P, SZ, P, P, P, P, P, P, SZ, P, P]
    modes = {"REF": ingress.REF, "WINDOW": ingress.WINDOW, "FULL": ingress.FULL}

    rows = []
    rng = np.random.default_rng(1)
    for name, lens in (("64B", np.full(n, 64)),
                       ("IMIX", rng.choice([64, 570, 1518], n, p=[7 / 12, 4 / 12, 1 / 12]))):
        pool = make_pool(n, lens, 5)
        slots = rng.permutation(n).astype(np.uint32)
        quads = (lens[slots].astype(np.int64) + 15) & ~15
        must = {"REF": n * (36 + 32),
                "WINDOW": n * 36 + int(np.minimum(quads, HDR_WINDOW).sum()) + n * HDR_WINDOW,
                "FULL": n * 36 + 2 * int(quads.sum())}
        need = int(quads.sum())
        w = gpu.GpuWorker(0, 16)
        d_pool = w.malloc(pool.size)
        w.h2d(d_pool, pool)
        pin = gpu.PinnedArray((pool.size,), np.uint8)
        pin.array[:] = pool
        d_slot = w.malloc(4 * n)
        w.h2d(d_slot, slots)
        room = max(need, n * HDR_WINDOW)
        d_out, d_copy = w.malloc(room), w.malloc(max(must.values()))
        d_desc, d_ts, d_ctrl, d_info = w.malloc(8 * n), w.malloc(8 * n), w.malloc(4 * n), w.malloc(64)
        w.sync()
        for where, src, which in (("hbm", d_pool, ("REF", "WINDOW", "FULL")),
                                  ("pinned", pin.ptr, ("WINDOW", "REF"))):
            for mname in which:
                mode = modes[mname]
                out = None if mname == "REF" else d_out
                out_bytes = 0 if mname == "REF" else room

                def gather(count=n):
                    w.ingress_gather(src, pool.size, STRIDE, d_slot, count, mode, d_desc, d_info,
                                     out=out, out_bytes=out_bytes, timestamp=d_ts, ctrl=d_ctrl)

                # the first 65536 handles against the host restatement
                k = min(n, 1 << 16)
                gather(k)
                got_info = w.fetch_ingress_info(d_info)
                want = ingress.gather_host(pool, STRIDE, slots[:k], mode)
                got = [np.zeros(int(want[4]["bytes"]), np.uint8), np.zeros(k, np.uint64),
                       np.zeros(k, np.uint64)]
                for host, dev in zip(got, (d_out, d_desc, d_ts)):
                    if host.size:
                        w.d2h(host, dev)
                w.sync()
                assert got_info == want[4], (got_info, want[4])
                assert all(np.array_equal(x, y) for x, y in zip(got, want[:3])), (where, mname)

                ms = (ctypes.c_float * 4)()
                passes = []
                for j in range(5 + reps):
                    rc = timed(w._ctx, src, pool.size, STRIDE, d_slot, n, mode, out, out_bytes,
                               d_desc, d_ts, d_ctrl, d_info, src, d_copy, must[mname], None, ms)
                    if rc != 0:
                        raise RuntimeError(gpu.LIB.upe_gpu_last_error().decode())
                    if j >= 5:
                        passes.append(tuple(ms))
                med = [1e3 * statistics.median(p[j] for p in passes) for j in range(4)]
                info = w.fetch_ingress_info(d_info)
                assert int(info["packed"]) == n and int(info["bad"]) == 0
                w.sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    gather()
                w.sync()
                whole = 1e6 * (time.perf_counter() - t0) / reps
                total = sum(med[:3])
                row = {"workload": name, "pool": where, "mode": mname, "n": n,
                       "must_bytes": must[mname],
                       "size_us": round(med[0], 1), "scan_us": round(med[1], 1),
                       "write_us": round(med[2], 1), "passes_us": round(total, 1),
                       "passes_GBps": round(must[mname] / total / 1e3, 1),
                       "ns_per_packet": round(1e3 * total / n, 3),
                       "copy_us": round(med[3], 1),
                       "copy_GBps": round(must[mname] / med[3] / 1e3, 1),
                       "passes_over_copy": round(total / med[3], 2),
                       "call_us": round(whole, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        for p in (d_pool, d_slot, d_out, d_copy, d_desc, d_ts, d_ctrl, d_info):
            w.free(p)
        pin.free()
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ingress_gather_time.py", "device": "MI355X", "stride": STRIDE,
                   "rows": rows}, f, indent=1)
        f.write("\n")
    assert INGRESS_INFO_DTYPE.itemsize == 64


if __name__ == "__main__":
    main()

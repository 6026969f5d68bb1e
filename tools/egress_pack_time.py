"""Time of upe_gpu_egress_pack's three passes (size, scan, copy) on GPU 0, beside the floor of the
copy pass — a plain device-to-device copy of the packed bytes on the same stream in the same run —
and what the pack saves a device-resident TX path: a device-to-host copy of the whole ingress
buffer against one of info.bytes.  All in one process.

  python tools/egress_pack_time.py [--out profiles/egress_pack.json] [--n 1048576]
                                   [--n-imix 262144] [--reps 30]

Workloads: synth.config_b(n, seed=2) (64-byte UDP frames) and synth.config_c_flows(n_imix) (IMIX
64/570/1518, IPv4 and IPv6), each classified on the device first, in place (pack with
d_hdr = NULL) and in emit mode on a second copy (pack with the records).
Per pass: HIP events around each launch (upe_gpu_egress_pack_timed), median of --reps packs after
5 warm-up ones; d2d_ms: hipMemcpyAsync of info.bytes between two events, the same calls.
pack_ms: a host clock around --reps back-to-back asynchronous packs ending in a synchronise, per
pack (no events between the launches).  d2h_*_ms: a host clock around one copy into pinned host
memory and a synchronise (median of 5).  host_ms: one egress.pack_host.  The device
result is checked against egress.pack_host before timing."""
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
    from upe_amd import egress, gpu, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egress_pack.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--n-imix", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    reps = args.reps

    P, SZ = ctypes.c_void_p, ctypes.c_size_t
    timed = gpu.LIB.upe_gpu_egress_pack_timed
    timed.restype = ctypes.c_int
    timed.argtypes = [P, P, P, P, P, SZ, P, SZ, P, P, P, P, P, P]

    rows = []
    for name, make in (("B", lambda: synth.config_b(n=args.n, seed=2)),
                       ("IMIX", lambda: synth.config_c_flows(n=args.n_imix))):
        wl = make()
        n = wl.n
        for mode in ("in_place", "emit"):
            w = gpu.GpuWorker(0, wl.capacity)
            w.configure(wl)
            b = gpu.DeviceBatch(w, wl.frames, wl.desc)
            if mode == "emit":
                b.run_emit()
            else:
                b.run()
            frames, verdict = b.fetch()
            rec = b.fetch_hdr(raw=True) if mode == "emit" else None
            t0 = time.perf_counter()
            want = egress.pack_host(frames, wl.desc, verdict, hdr=rec)
            t_host = 1e3 * (time.perf_counter() - t0)
            need = int(want[3]["need"])
            out, copy = w.malloc(max(need, 16)), w.malloc(max(need, 16))
            out_desc, out_index, info = w.malloc(8 * n), w.malloc(4 * n), w.malloc(32)

            def pack():
                w.egress_pack(b.frames, b.desc, b.verdict, n, out, need, out_desc, info,
                              hdr=b.hdr or None, out_index=out_index)

            pack()
            got_info = w.fetch_egress_info(info)
            packed = int(got_info["packed"])
            got = [np.zeros(need, np.uint8), np.zeros(packed, np.uint64),
                   np.zeros(packed, np.uint32)]
            for host, dev in zip(got, (out, out_desc, out_index)):
                if host.size:
                    w.d2h(host, dev)
            w.sync()
            assert got_info == want[3], (got_info, want[3])
            assert all(np.array_equal(x, y) for x, y in zip(got, want[:3]))

            ms = (ctypes.c_float * 4)()
            passes = []
            for k in range(5 + reps):
                rc = timed(w._ctx, b.frames, b.desc, b.verdict, b.hdr or None, n, out, need,
                           out_desc, out_index, info, copy, None, ms)
                if rc != 0:
                    raise RuntimeError(gpu.LIB.upe_gpu_last_error().decode())
                if k >= 5:
                    passes.append(tuple(ms))
            med = [statistics.median(p[j] for p in passes) for j in range(4)]
            w.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                pack()
            w.sync()
            whole = 1e3 * (time.perf_counter() - t0) / reps

            pin = gpu.PinnedArray((max(b.frames_nbytes, need, 1),), np.uint8)
            d2h = {}
            for what, src, size in (("ingress", b.frames, b.frames_nbytes), ("packed", out, need)):
                t = []
                for _ in range(5):
                    w.sync()
                    t0 = time.perf_counter()
                    if size:
                        w.d2h(pin.array[:size], src)
                    w.sync()
                    t.append(1e3 * (time.perf_counter() - t0))
                d2h[what] = statistics.median(t)
            pin.free()

            row = {"workload": name, "mode": mode, "n": n, "forwarded": int(got_info["frames"]),
                   "ingress_bytes": b.frames_nbytes, "packed_bytes": need,
                   "size_ms": round(med[0], 4), "scan_ms": round(med[1], 4),
                   "copy_ms": round(med[2], 4), "passes_ms": round(sum(med[:3]), 4),
                   "d2d_ms": round(med[3], 4),
                   "copy_over_d2d": round(med[2] / med[3], 2) if med[3] > 0 else None,
                   "copy_pass_GBps": round(2 * need / med[2] / 1e6, 1) if med[2] > 0 else None,
                   "pack_ms": round(whole, 4),
                   "d2h_ingress_ms": round(d2h["ingress"], 3),
                   "d2h_packed_ms": round(d2h["packed"], 3),
                   "host_ms": round(t_host, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            for p in (out, copy, out_desc, out_index, info):
                w.free(p)
            b.free()
            w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/egress_pack_time.py", "device": "MI355X", "rows": rows}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Time of upe_gpu_release_order on GPU 0, beside a device-to-device copy of the bytes the call
must move, taken on the same stream in the same run, and of the host's upe_release_flush over the
fetched lists.  All in one process.

  python tools/release_order_time.py [--out profiles/release_order.json] [--reps 30]

Rows: 1M and 65536 packets of synth.config_b (config B's forwarded density) and of
synth.config_c_flows (the IMIX leg's), classified on the device first, so the verdict words are a
launch's own; bursts of 32 (the fixed form) and of varying size (an offset array, lengths cycling
1..64); handles (a permutation), the reply list and the info all asked for.
call_us: HIP events (torch.cuda.Event) on one stream around the call — its three launches — the
median of --reps calls after 5 warm-up ones; copy_us: one copy of must_bytes between two events on
the same stream, the same way.
must_bytes: 4 read per packet (the verdict word) plus 4 per written output entry (order, handle,
one count per burst, the replies).  The call also reads the handles (4 per packet) and, in the
offset form, the offsets (4 per burst): read_also_bytes.
flush_ns_per_packet: upe_release_flush over the lists copied to the host with callbacks that do
nothing (compiled C, so that the time is the function's own), a host clock around --reps calls.
The device's lists of the timed calls are checked against release.order_host."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOOPS = r"""
#include <stddef.h>
#include <stdint.h>
int send_one(void *u, const uint8_t *f, size_t len) { (void)u, (void)f, (void)len; return 0; }
int send(void *u, const uint8_t *const *f, const size_t *l, int c) {
    (void)u, (void)f, (void)l;
    return c;
}
void release(void *u, const uint32_t *h, size_t c) { (void)u, (void)h, (void)c; }
"""


def noop_ops(gpu, d):
    src, lib = os.path.join(d, "noops.c"), os.path.join(d, "noops.so")
    with open(src, "w") as f:
        f.write(NOOPS)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", lib, src], check=True)
    so = ctypes.CDLL(lib)
    cast = lambda fn, t: ctypes.cast(fn, t)
    return so, gpu.ReleaseOps(cast(so.send_one, gpu.TX_SEND_FN), cast(so.send, gpu.TX_BATCH_FN),
                              cast(so.release, gpu.RELEASE_FN))


def main() -> None:
    import torch

    from upe_amd import gpu, release, synth
    from upe_amd.layout import RELEASE_INFO_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "release_order.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    reps = args.reps

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        so, ops = noop_ops(gpu, tmp)
        for name, make in (("B", synth.config_b), ("CF", synth.config_c_flows)):
            for n in (1 << 20, 1 << 16):
                wl = make(n=n)
                w = gpu.GpuWorker(0, wl.capacity)
                w.configure(wl)
                b = gpu.DeviceBatch(w, wl.frames, wl.desc)
                b.run_emit()
                frames, verdict = b.fetch()
                slot = np.random.default_rng(n).permutation(n).astype(np.uint32)
                cycle = [0]
                while cycle[-1] < n:
                    cycle.append(min(n, cycle[-1] + 1 + (len(cycle) - 1) % 64))
                for form, first in (("fixed 32", None),
                                    ("cycling 1..64", np.array(cycle, np.uint32))):
                    exp = release.order_host(verdict, first=first, burst=None if first is not None
                                             else 32, slot=slot)
                    nb, replies = len(exp.burst_fwd), len(exp.reply)
                    must = 4 * n + 4 * (2 * n + nb + replies)
                    also = 4 * n + (4 * (nb + 1) if first is not None else 0)
                    d_slot, d_first = w.malloc(4 * n), w.malloc(4 * (nb + 1))
                    w.h2d(d_slot, slot)
                    if first is not None:
                        w.h2d(d_first, first)
                    d_order, d_handle, d_reply = (w.malloc(4 * n) for _ in range(3))
                    d_bf, d_info = w.malloc(4 * nb), w.malloc(64)
                    src = torch.empty(must, dtype=torch.uint8, device="cuda:0")
                    dst = torch.empty(must, dtype=torch.uint8, device="cuda:0")
                    w.sync()
                    took, copy = [], []
                    for j in range(5 + reps):
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                        ev[0].record(stream)
                        w.release_order(b.verdict, n, d_order, d_bf, d_info,
                                        first=d_first if first is not None else None,
                                        nb=nb if first is not None else 0,
                                        burst=0 if first is not None else 32, slot=d_slot,
                                        handle=d_handle, reply=d_reply, stream=s)
                        ev[1].record(stream)
                        ev[2].record(stream)
                        with torch.cuda.stream(stream):
                            dst.copy_(src, non_blocking=True)
                        ev[3].record(stream)
                        ev[3].synchronize()
                        if j >= 5:
                            took.append(1e3 * ev[0].elapsed_time(ev[1]))
                            copy.append(1e3 * ev[2].elapsed_time(ev[3]))
                    order, handle = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
                    bf, reply = np.zeros(nb, np.uint32), np.zeros(max(replies, 1), np.uint32)
                    info = np.zeros(1, RELEASE_INFO_DTYPE)
                    for h, p in ((order, d_order), (handle, d_handle), (bf, d_bf), (reply, d_reply),
                                 (info, d_info)):
                        w.d2h(h, p)
                    w.sync()
                    reply = reply[:replies]
                    assert info[0].tobytes() == exp.info.tobytes(), (info, exp.info)
                    assert np.array_equal(order, exp.order) and np.array_equal(handle, exp.handle)
                    assert np.array_equal(bf, exp.burst_fwd) and np.array_equal(reply, exp.reply)
                    # the host flush over those lists, nothing done in the callbacks
                    P = gpu._np_ptr
                    fwd, drp = ctypes.c_uint64(0), ctypes.c_uint64(0)
                    flush = lambda: gpu.LIB.upe_release_flush(
                        P(frames), P(wl.desc), P(order), P(handle),
                        P(first) if first is not None else None, nb,
                        0 if first is not None else 32, n, P(bf), P(reply) if replies else None,
                        replies, ctypes.byref(ops), None, ctypes.byref(fwd), ctypes.byref(drp))
                    assert flush() == 0
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        flush()
                    flush_ns = 1e9 * (time.perf_counter() - t0) / reps / n
                    assert fwd.value == (reps + 1) * int(exp.info["forwarded"]) and drp.value == 0
                    med, cmed = statistics.median(took), statistics.median(copy)
                    row = {"config": name, "n": n, "bursts": form, "nb": nb,
                           "forwarded": round(int(exp.info["forwarded"]) / n, 4),
                           "replies": replies, "must_bytes": must, "read_also_bytes": also,
                           "call_us": round(med, 1), "call_min_us": round(min(took), 1),
                           "call_GBps": round(must / med / 1e3, 1),
                           "call_ns_per_packet": round(1e3 * med / n, 4),
                           "copy_us": round(cmed, 1), "copy_GBps": round(must / cmed / 1e3, 1),
                           "call_over_copy": round(med / cmed, 2),
                           "flush_ns_per_packet": round(flush_ns, 2)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    for p in (d_slot, d_first, d_order, d_handle, d_reply, d_bf, d_info):
                        w.free(p)
                b.free()
                w.close()
        del ops, so
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/release_order_time.py", "device": "MI355X",
                   "block": gpu.RELEASE_BLOCK, "reps": reps, "runs": 1, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

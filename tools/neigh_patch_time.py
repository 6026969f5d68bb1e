"""Times on GPU 0, all in one process:

1. upe_gpu_neigh_patch alone at 1, 1024 and 65536 records that refresh addresses of
   synth.config_b's ARP table: HIP events (torch.cuda.Event) on one stream around the call — its
   launches and the L1 agreement launches behind them — the median of --reps calls after 5 warm-up
   ones.
2. A synth.config_b batch of --n packets carrying 0, 16 and 256 ARP packets from addresses the
   table holds (refreshes, evenly spread, new MACs) through upe_gpu_process_segmented and through
   upe_gpu_process_segmented_resident.  Both calls are synchronous and rewrite the frames in place,
   so every call gets the frames uploaded again and a fresh copy of the host slot arrays first,
   outside the clock; the clock is the host's (time.perf_counter) around the call, the two calls
   alternate within a repetition on one context, median of --reps after 5 warm-up pairs.  The
   existing call is the yardstick: ratio = resident / segmented.  The two calls' verdicts are
   compared once per row.

  python tools/neigh_patch_time.py [--out profiles/neigh_patch.json] [--n 65536] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # ctrl_cases: a generator module, not a test


def with_refreshes(wl, k, synth, rows_of):
    """wl with k ARP packets from addresses its ARP table holds, evenly spread, new MACs."""
    if k == 0:
        return wl
    h, lens = rows_of(wl)
    known = wl.arp["ip"][wl.arp["valid"] != 0]
    every = wl.n // k
    rows, lns, src = [], [], 0
    for j in range(k):
        p = j * every
        rows.append(h[src:p])
        lns.append(lens[src:p])
        f = synth._frame(synth._eth(0x0806, dst=b"\xff" * 6),
                         synth._arp(1, bytes([0x0C, j >> 8, j & 0xFF, 1, 2, 3]),
                                    int(known[(j * 7919) % len(known)]), bytes(6), 0x0A800001))
        r = np.zeros((1, 128), np.uint8)
        r[0, :len(f)] = np.frombuffer(f, np.uint8)
        rows.append(r)
        lns.append(np.array([len(f)], np.int64))
        src = p
    rows.append(h[src:])
    lns.append(lens[src:])
    frames, desc = synth.pack_frames(np.concatenate(rows), np.concatenate(lns))
    return synth.Workload(wl.name + "+refresh", frames, desc, wl.rules, wl.capacity,
                          wl.arp.copy(), wl.ndp.copy(), wl.eth_addr, wl.ip4_addr, wl.l1.copy())


def main() -> None:
    import torch

    import ctrl_cases
    from upe_amd import gpu, synth
    from upe_amd.layout import CTRL_WRITE_DTYPE, CW_ARP, PATCH_INFO_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neigh_patch.json"))
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n, reps = args.n, args.reps

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    base = synth.config_b(n=n)
    known = base.arp["ip"][base.arp["valid"] != 0]

    # 1. the patch alone
    alone = []
    w = gpu.GpuWorker(0, base.capacity)
    w.configure(base)
    for count in (1, 1024, 65536):
        recs = np.zeros(count, CTRL_WRITE_DTYPE)
        recs["index"] = np.arange(count)
        recs["kind"] = CW_ARP
        recs["mac_off"] = 22
        recs["mac"][:, 0] = 0x0E
        recs["mac"][:, 1:5] = np.arange(count, dtype="<u4").view(np.uint8).reshape(-1, 4)
        recs["ip"][:, :4] = known[np.arange(count) % len(known)].astype("<u4").view(
            np.uint8).reshape(-1, 4)
        d_w, d_i = w.malloc(32 * count), w.malloc(32)
        w.h2d(d_w, recs.view(np.uint8).ravel())
        w.sync()
        took = []
        for j in range(5 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            w.neigh_patch(d_w, count, None, d_i, stream=s)
            e1.record(stream)
            e1.synchronize()
            if j >= 5:
                took.append(1e3 * e0.elapsed_time(e1))
        info = np.zeros(1, PATCH_INFO_DTYPE)
        w.d2h(info, d_i)
        w.sync()
        assert int(info["patched"][0]) == count, info
        row = {"records": count, "distinct_slots": int(min(count, len(known))),
               "patch_us": round(statistics.median(took), 1), "patch_min_us": round(min(took), 1)}
        alone.append(row)
        print(json.dumps(row), flush=True)
        w.free(d_w)
        w.free(d_i)
    w.close()

    # 2. the two segmented calls
    rows = []
    for k in (0, 16, 256):
        wl = with_refreshes(base, k, synth, ctrl_cases._rows)
        w = gpu.GpuWorker(0, wl.capacity)
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        took = {"segmented": [], "resident": []}
        verdicts, infos = {}, {}
        for j in range(5 + reps):
            for name in took:
                w.load_neigh(wl.arp, wl.ndp)
                w.set_l1(wl.l1)
                w.h2d(b.frames, wl.frames)
                w.sync()
                arp, ndp = wl.arp.copy(), wl.ndp.copy()
                t0 = time.perf_counter()
                if name == "segmented":
                    infos[name] = w.process_segmented(b.frames, b.desc, b.verdict, b.n, arp, ndp,
                                                      now=1)
                else:
                    infos[name] = w.process_segmented_resident(b.frames, b.desc, b.verdict, b.n,
                                                               arp, ndp, now=1)
                t1 = time.perf_counter()
                if j >= 5:
                    took[name].append(1e6 * (t1 - t0))
                verdicts[name] = b.fetch()[1]
        assert np.array_equal(verdicts["segmented"], verdicts["resident"]), k
        ri = infos["resident"]
        assert int(ri["writes"]) == infos["segmented"] == k, (k, ri)
        med = {name: statistics.median(v) for name, v in took.items()}
        row = {"config": "B", "n": wl.n, "refresh_arp_packets": k,
               "patched": int(ri["patched"]), "rebuilds": int(ri["rebuilds"]),
               "segmented_us": round(med["segmented"], 1),
               "segmented_min_us": round(min(took["segmented"]), 1),
               "resident_us": round(med["resident"], 1),
               "resident_min_us": round(min(took["resident"]), 1),
               "resident_over_segmented": round(med["resident"] / med["segmented"], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        b.free()
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/neigh_patch_time.py", "device": "MI355X", "reps": reps,
                   "patch_alone": alone, "segmented_runs": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Times on GPU 0, all in one process: upe_gpu_neigh_learn of 1, 64 and 1024 NEW ARP addresses
into synth.config_b's snapshot compiled with room (upe_neigh_compile_room), against the only route
these records had before it: upe_neigh_apply_writes on the host slot arrays, upe_gpu_load_neigh,
upe_gpu_sync.

Every timed call starts from the same state: the image is loaded again (the learn) or the slot
arrays copied again (the yardstick) outside the clock.  The clock is the host's
(time.perf_counter) around the call and the upe_gpu_sync behind it, for both routes; the learn's
device time (HIP events on its stream around the call: its launch and the L1 agreement launches
behind it) is reported beside it.  The two routes alternate within a repetition on one context;
medians of --reps after 5 warm-up pairs.  Config B's ARP table has fewer than 1024 invalid
slots: the addresses past them meet a full table on both routes (dropped).  Once per row the
learn's answers for the new addresses are compared with the yardstick's.

  python tools/neigh_learn_time.py [--out profiles/neigh_learn.json] [--reps 20]
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


def main() -> None:
    import torch

    from upe_amd import gpu, synth
    from upe_amd.layout import CTRL_WRITE_DTYPE, CW_ARP, FLOW_KEY_DTYPE, LEARN_INFO_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neigh_learn.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = args.reps

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    base = synth.config_b(n=4096)
    held = set(int(x) for x in base.arp["ip"][base.arp["valid"] != 0])
    free = int((base.arp["valid"] == 0).sum())
    w = gpu.GpuWorker(0, base.capacity)
    w.configure(base)
    rows = []
    for count in (1, 64, 1024):
        took_in = min(count, free)   # the table's invalid slots: past them it is full, and drops
        new, a = [], 0xC0A90000
        while len(new) < count:
            a += 1
            if a not in held:
                new.append(a)
        recs = np.zeros(count, CTRL_WRITE_DTYPE)
        recs["index"] = np.arange(count)
        recs["kind"] = CW_ARP
        recs["mac_off"] = 22
        recs["mac"][:, 0] = 0x0E
        recs["mac"][:, 1:5] = np.arange(count, dtype="<u4").view(np.uint8).reshape(-1, 4)
        recs["ip"][:, :4] = np.array(new, "<u4").view(np.uint8).reshape(-1, 4)
        keys = np.zeros(count, FLOW_KEY_DTYPE)
        keys["ip_ver"] = 4
        keys["dst_ip"][:, :4] = recs["ip"][:, :4]
        # room enough that every new address finds a free candidate slot
        image = gpu.NeighImage(base.arp, base.ndp, room=(16 * count, 0))
        d_w, d_i = w.malloc(32 * count), w.malloc(64)
        d_k, d_m = w.malloc(keys.nbytes), w.malloc(8 * count)
        w.h2d(d_w, recs.view(np.uint8).ravel())
        w.h2d(d_k, keys.view(np.uint8).ravel())
        w.sync()
        took = {"learn": [], "learn_dev": [], "rebuild": []}
        answers = {}
        info = np.zeros(1, LEARN_INFO_DTYPE)
        for j in range(5 + reps):
            # the device route
            w.load_neigh_image(image)
            w.sync(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            w.neigh_learn(d_w, count, None, d_i, stream=s)
            e1.record(stream)
            w.sync(s)
            t1 = time.perf_counter()
            e1.synchronize()
            if j >= 5:
                took["learn"].append(1e6 * (t1 - t0))
                took["learn_dev"].append(1e3 * e0.elapsed_time(e1))
            w.d2h(info.view(np.uint8).ravel(), d_i)
            w.sync()
            assert int(info["inserted"][0]) == took_in and int(info["deferred"][0]) == 0, info
            assert int(info["dropped"][0]) == count - took_in, info
            got = np.zeros(count, np.uint64)
            w.resolve_keys(d_k, count, d_m)
            w.d2h(got, d_m)
            w.sync()
            answers["learn"] = got
            # the host route: the parent's only one for a new address
            arp, ndp = base.arp.copy(), base.ndp.copy()
            w.load_neigh(arp, ndp)
            w.sync()
            t0 = time.perf_counter()
            gpu.neigh_apply_writes(arp, ndp, recs, now=1)
            w.load_neigh(arp, ndp)
            w.sync()
            t1 = time.perf_counter()
            if j >= 5:
                took["rebuild"].append(1e6 * (t1 - t0))
            got = np.zeros(count, np.uint64)
            w.resolve_keys(d_k, count, d_m)
            w.d2h(got, d_m)
            w.sync()
            answers["rebuild"] = got
        assert np.array_equal(answers["learn"], answers["rebuild"])
        assert int((answers["learn"] != 0).sum()) == took_in
        med = {k: statistics.median(v) for k, v in took.items()}
        row = {"config": "B", "new_arp_addresses": count, "arp_room": 16 * count,
               "inserted": took_in, "dropped_table_full": count - took_in,
               "learn_us": round(med["learn"], 1), "learn_min_us": round(min(took["learn"]), 1),
               "learn_device_us": round(med["learn_dev"], 1),
               "rebuild_us": round(med["rebuild"], 1),
               "rebuild_min_us": round(min(took["rebuild"]), 1),
               "learn_over_rebuild": round(med["learn"] / med["rebuild"], 3),
               "learn_us_per_record": round(med["learn"] / count, 2),
               "rebuild_us_per_record": round(med["rebuild"] / count, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (d_w, d_i, d_k, d_m):
            w.free(p)
        image.free()
    w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/neigh_learn_time.py", "device": "MI355X", "reps": reps,
                   "yardstick": "upe_neigh_apply_writes + upe_gpu_load_neigh + upe_gpu_sync",
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Times of upe_gpu_resolve_keys on GPU 0 at --n keys cut from the destinations of configs B and
C6 (config C with IPv6 forwarding: both neighbour tables are asked), beside upe_gpu_match_keys over
the same keys on the same stream in the same run.  All in one process.

  python tools/resolve_keys_time.py [--out profiles/resolve_keys.json] [--n 1048576] [--reps 20]

The keys are upe_gpu_parse_keys' of the config's frames.  Per call: HIP events (torch.cuda.Event)
on one stream around the call, the median of --reps calls after 5 warm-up ones; the two calls
alternate within a repetition, so that clock and cache state drift hits them alike.  dry_run_us: a
host clock around upe_gpu_resolve_keys with a compiled image (upload, launch, synchronise, free),
median of 5; compile_us: a host clock around upe_neigh_compile, median of 5.
must_bytes: resolve reads 44 bytes per key and writes 8 (the index slots it reads are not
counted); match reads 44 and writes 4.
The answers are checked against upe_neigh_lookup_host (all keys) and neigh.resolve_keys (the first
65536)."""
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

    from upe_amd import gpu, neigh, synth
    from upe_amd.layout import FLOW_KEY_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolve_keys.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="B,C6")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    make = {"B": lambda: synth.config_b(n=n),
            "C6": lambda: synth.config_c(n=n, v6_forwarding=True)}

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rows = []
    for name in args.configs.split(","):
        wl = make[name]()
        w = gpu.GpuWorker(0, wl.capacity)
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        d_keys, d_mac, d_rule = w.malloc(44 * n), w.malloc(8 * n), w.malloc(4 * n)
        w.parse_keys(b.frames, b.desc, n, d_keys, None, s)
        w.sync(s)
        calls = {
            "resolve_keys": lambda: w.resolve_keys(d_keys, n, d_mac, stream=s),
            "match_keys": lambda: w.match_keys(d_keys, n, d_rule, stream=s),
        }
        took = {k: [] for k in calls}
        for j in range(5 + reps):
            for k, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if j >= 5:
                    took[k].append(1e3 * e0.elapsed_time(e1))
        w.sync(s)
        keys = np.empty(n, FLOW_KEY_DTYPE)
        mac = np.empty(n, np.uint64)
        w.d2h(keys.view(np.uint8).reshape(-1), d_keys)
        w.d2h(mac, d_mac)
        w.sync()
        want = gpu.neigh_lookup_host(wl.arp, wl.ndp, keys)
        assert np.array_equal(mac, want), name
        assert np.array_equal(neigh.resolve_keys(wl.arp, wl.ndp, keys[:65536]), want[:65536]), name
        comp, dry = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            image = gpu.NeighImage(wl.arp, wl.ndp)
            t1 = time.perf_counter()
            w.resolve_keys(d_keys, n, d_mac, image=image, stream=s)
            t2 = time.perf_counter()
            comp.append(1e6 * (t1 - t0))
            dry.append(1e6 * (t2 - t1))
            image.free()
        w.d2h(mac, d_mac)
        w.sync()
        assert np.array_equal(mac, want), name + " (dry run)"
        med = {k: statistics.median(v) for k, v in took.items()}
        row = {"config": name, "n": n,
               "arp_slots": int(len(wl.arp)), "arp_valid": int((wl.arp["valid"] != 0).sum()),
               "ndp_slots": int(len(wl.ndp)), "ndp_valid": int((wl.ndp["valid"] != 0).sum()),
               "ipv4_keys": int((keys["ip_ver"] == 4).sum()),
               "ipv6_keys": int((keys["ip_ver"] == 6).sum()),
               "found": int((want != 0).sum()),
               "resolve_keys_us": round(med["resolve_keys"], 1),
               "resolve_keys_min_us": round(min(took["resolve_keys"]), 1),
               "resolve_must_bytes": 52 * n,
               "resolve_GBps": round(52 * n / med["resolve_keys"] / 1e3, 1),
               "match_keys_us": round(med["match_keys"], 1),
               "match_keys_min_us": round(min(took["match_keys"]), 1),
               "match_must_bytes": 48 * n,
               "match_GBps": round(48 * n / med["match_keys"] / 1e3, 1),
               "resolve_over_match": round(med["resolve_keys"] / med["match_keys"], 2),
               "compile_us": round(statistics.median(comp), 1),
               "dry_run_us": round(statistics.median(dry), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (d_keys, d_mac, d_rule):
            w.free(p)
        b.free()
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/resolve_keys_time.py", "device": "MI355X", "reps": reps,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

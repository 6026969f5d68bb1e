"""Times of upe_gpu_ctrl_writes on GPU 0 for synth.config_c at --n packets with 0, 1 % and 10 %
control packets inserted (tests/ctrl_cases.with_control, the generator of the segmented GPU test),
beside upe_gpu_parse_keys over the same batch on the same stream in the same run: a pass with a
comparable read pattern (every descriptor, each frame's first bytes).  All in one process.

  python tools/ctrl_writes_time.py [--out profiles/ctrl_writes.json] [--n 1048576] [--reps 20]

Per call: HIP events (torch.cuda.Event) on one stream around the call — all of its launches — the
median of --reps calls after 5 warm-up ones; the two calls alternate within a repetition, so that
clock and cache state drift hits them alike.  must_bytes: ctrl_writes reads 8 bytes of descriptor
and 12 frame bytes per packet and writes a 4-byte word to scratch, plus 32 bytes per record;
parse_keys reads the descriptor and writes a 44-byte key (the header bytes it reads are not
counted).  The records are checked against upe_ctrl_writes_host."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # ctrl_cases: a generator module, not a test


def main() -> None:
    import torch

    import ctrl_cases
    from upe_amd import gpu, synth
    from upe_amd.layout import CTRL_WRITE_DTYPE

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctrl_writes.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--percent", default="0,1,10")
    args = ap.parse_args()
    n, reps = args.n, args.reps

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    base = synth.config_c(n=n)
    rows = []
    for pc in (float(x) for x in args.percent.split(",")):
        k = int(round(n * pc / 100))
        wl = ctrl_cases.with_control(base, k, 31) if k else base
        m = len(wl.desc)
        want, winfo = gpu.ctrl_writes_host(wl.frames, wl.desc)
        cap = len(want) + 16
        w = gpu.GpuWorker(0, wl.capacity)
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        d_writes, d_info, d_keys = w.malloc(32 * cap), w.malloc(32), w.malloc(44 * m)
        calls = {
            "ctrl_writes": lambda: w.ctrl_writes(b.frames, b.desc, m, d_writes, cap, d_info,
                                                 stream=s),
            "parse_keys": lambda: w.parse_keys(b.frames, b.desc, m, d_keys, None, s),
        }
        took = {name: [] for name in calls}
        for j in range(5 + reps):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if j >= 5:
                    took[name].append(1e3 * e0.elapsed_time(e1))
        got, ginfo = w.fetch_ctrl_writes(d_writes, d_info, stream=s)
        assert ginfo.tobytes() == winfo.tobytes(), pc
        assert got.tobytes() == np.ascontiguousarray(want, CTRL_WRITE_DTYPE).tobytes(), pc
        med = {name: statistics.median(v) for name, v in took.items()}
        cw_bytes = 24 * m + 32 * len(want)
        row = {"config": "C", "percent_control": pc, "n": m, "inserted": k,
               "ctrl": int(winfo["ctrl"]), "writes": int(winfo["writes"]),
               "ctrl_writes_us": round(med["ctrl_writes"], 1),
               "ctrl_writes_min_us": round(min(took["ctrl_writes"]), 1),
               "ctrl_writes_must_bytes": cw_bytes,
               "ctrl_writes_GBps": round(cw_bytes / med["ctrl_writes"] / 1e3, 1),
               "parse_keys_us": round(med["parse_keys"], 1),
               "parse_keys_min_us": round(min(took["parse_keys"]), 1),
               "parse_keys_must_bytes": 52 * m,
               "parse_keys_GBps": round(52 * m / med["parse_keys"] / 1e3, 1),
               "ctrl_over_parse": round(med["ctrl_writes"] / med["parse_keys"], 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (d_writes, d_info, d_keys):
            w.free(p)
        b.free()
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ctrl_writes_time.py", "device": "MI355X", "reps": reps,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

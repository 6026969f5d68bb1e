"""Times of upe_gpu_parse_keys and upe_gpu_match_keys on GPU 0 at --n keys for the tables of
configs B, C and D, each beside upe_gpu_process over the frames that carry the same keys (the
fused classify launch: parse, match, rewrite, neighbour lookup, counters, rule_stats), on the same
stream in the same run.  All in one process.

  python tools/match_keys_time.py [--out profiles/match_keys.json] [--n 1048576] [--reps 20]

Per call: HIP events (torch.cuda.Event) on one stream around the call, the median of --reps calls
after 5 warm-up ones; the three calls alternate within a repetition, so that clock and cache state
drift hits them alike.  dry_run_us: a host clock around upe_gpu_match_keys with a compiled image
(upload, launch, synchronise, free), median of 5.
must_bytes: parse reads a descriptor and at most 96 frame bytes per packet and writes 44 + 4;
match reads 44 and writes 4.
The match results are checked against the rule index of upe_gpu_process's verdicts."""
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

    from upe_amd import gpu, layout, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_keys.json"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="B,C,D")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    make = {"B": lambda: synth.config_b(n=n), "C": lambda: synth.config_c(n=n),
            "D": lambda: synth.config_d(n=n)}

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rows = []
    for name in args.configs.split(","):
        wl = make[name]()
        w = gpu.GpuWorker(0, wl.capacity)
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        d_keys, d_rc, d_rule = w.malloc(44 * n), w.malloc(4 * n), w.malloc(4 * n)
        calls = {
            "parse_keys": lambda: w.parse_keys(b.frames, b.desc, n, d_keys, d_rc, s),
            "match_keys": lambda: w.match_keys(d_keys, n, d_rule, stream=s),
            "process": lambda: w.process(b.frames, b.desc, b.verdict, n, s),
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
        rule = np.empty(n, np.int32)
        verdict = np.empty(n, np.uint32)
        w.d2h(rule, d_rule)
        w.d2h(verdict, b.verdict)
        w.sync()
        assert np.array_equal(rule, layout.verdict_rule(verdict)), name
        image = gpu.RuleImage(wl.rules_sorted, wl.capacity)
        dry = []
        for _ in range(5):
            t0 = time.perf_counter()
            w.match_keys(d_keys, n, d_rule, image=image, stream=s)
            dry.append(1e6 * (time.perf_counter() - t0))
        w.d2h(rule, d_rule)
        w.sync()
        assert np.array_equal(rule, layout.verdict_rule(verdict)), name + " (dry run)"
        image.free()
        med = {k: statistics.median(v) for k, v in took.items()}
        lens = np.minimum(layout.desc_lens(wl.desc), 96)
        parse_bytes = int(8 * n + ((lens + 15) // 16 * 16).sum() + 48 * n)
        row = {"config": name, "n": n, "rules": int(len(wl.rules_sorted)),
               "index_kind": w.rule_index_kind(), "matched": int((rule >= 0).sum()),
               "parse_keys_us": round(med["parse_keys"], 1),
               "parse_keys_min_us": round(min(took["parse_keys"]), 1),
               "parse_must_bytes": parse_bytes,
               "parse_GBps": round(parse_bytes / med["parse_keys"] / 1e3, 1),
               "match_keys_us": round(med["match_keys"], 1),
               "match_keys_min_us": round(min(took["match_keys"]), 1),
               "match_must_bytes": 48 * n,
               "match_GBps": round(48 * n / med["match_keys"] / 1e3, 1),
               "process_us": round(med["process"], 1),
               "process_min_us": round(min(took["process"]), 1),
               "parse_plus_match_over_process": round(
                   (med["parse_keys"] + med["match_keys"]) / med["process"], 2),
               "dry_run_us": round(statistics.median(dry), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (d_keys, d_rc, d_rule):
            w.free(p)
        b.free()
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/match_keys_time.py", "device": "MI355X", "reps": reps,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

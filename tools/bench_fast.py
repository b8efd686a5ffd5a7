#!/usr/bin/env python3
"""Exact against fast encode (mode="fast", fast parse v1), device-resident.

For 4 GiB of G1 int16 and for G2 float32 at the largest power-of-two size up
to 16 GiB that fits the device, compresses the same tensor in both modes,
alternating exact / fast step by step in one process after a warm-up, each
step timed with device events.  Prints one JSON line per input and mode (GiB/s
of uncompressed bytes from the median step, ms per step with min / max as the
spread, stream bytes) and one line per input with the fast / exact ratios.
The fast stream is decoded once and compared with the input before timing.

  python tools/bench_fast.py [--steps 7] [--warmup 2] [--gib-g1 4] [--gib-g2 0]

For the kernel times, run it under the profiler on its own, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_fast.py --steps 3 --gib-g1 1 --gib-g2 1
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GIB = 1 << 30


def run_input(torch, B, name, gen, dtype, gib, steps, warmup):
    api = B.api
    es = torch.empty(0, dtype=dtype).element_size()
    n = int(gib * GIB) // es // 8 * 8
    x = torch.empty(n, dtype=dtype, device="cuda")
    B.synth_fill_dev(x, gen, first=0, seed=12345)
    comp = torch.empty(B.compress_lz4_bound(n, es, 0), dtype=torch.uint8, device="cuda")
    ws = api.compress_lz4_workspace(n, es, 0)
    res = torch.empty(1, dtype=torch.int64, device="cuda")
    modes = ("exact", "fast")

    def step(mode):
        api.compress_lz4_dev(x, out=comp, workspace=ws, result=res, sync=False, mode=mode)

    # the fast stream is a stream: the decoder returns the input
    step("fast")
    c = int(res.item())
    y = api.decompress_lz4_dev(comp[:c], x.shape, dtype)
    if not torch.equal(x, y):
        raise SystemExit("%s: the fast stream does not decode to the input" % name)
    del y
    size = {}
    for _ in range(warmup):
        for m in modes:
            step(m)
            size[m] = int(res.item())
    ev = {m: [] for m in modes}
    for _ in range(steps):
        for m in modes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(m)
            b.record()
            ev[m].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for m in modes:
        ms = [a.elapsed_time(b) for a, b in ev[m]]
        med = statistics.median(ms)
        out[m] = med
        print(json.dumps({"input": name, "mode": m, "gib": n * es / GIB, "steps": steps,
                          "gib_per_s": round(n * es / GIB / (med / 1e3), 2),
                          "ms_per_step": round(med, 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4), "stream_bytes": size[m]}), flush=True)
    print(json.dumps({"input": name, "fast_over_exact_speed": round(out["exact"] / out["fast"], 3),
                      "fast_over_exact_size": round(size["fast"] / size["exact"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=7, help="timed steps per mode (>= 5 for a record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gib-g1", type=float, default=4.0)
    ap.add_argument("--gib-g2", type=float, default=0.0, help="0: the largest of 16, 8, 4, ... that fits")
    args = ap.parse_args()
    import torch

    import bitshuffle_amd as B
    if not B.using_HIP():
        raise SystemExit("no HIP device")
    g2 = args.gib_g2
    if not g2:
        free = torch.cuda.mem_get_info()[0]
        g2 = 16.0
        # input + output bound + scratch slots + decoded copy of the check
        while g2 > 0.25 and 4.5 * g2 * GIB > free:
            g2 /= 2
    run_input(torch, B, "G1 int16", 1, torch.int16, args.gib_g1, args.steps, args.warmup)
    run_input(torch, B, "G2 float32", 2, torch.float32, g2, args.steps, args.warmup)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Ragged window decode against what a caller had before it, device-resident.

The stream and the windows of tools/window_decode_bench.py: one G1 int16
stream (synth_fill_dev, default block size, --gib of raw data) with its block
index, and 4096 windows at odd starts, at most 65,536 elements long.

  r  decompress_lz4_ragged_dev, counts uniform in [1, 65536], packed output
  p  decompress_lz4_windows_dev with every window padded to 65,536 elements:
     what a caller with variable lengths had to do (and then compact the result)
  q  decompress_lz4_ragged_dev with every count = 65,536: the same work as p,
     plus the placement scan and the per-window lengths

All with a caller workspace, output, offsets, result and the index supplied.
The cases named in --cases are timed in ONE loop, alternating, each call
between two device events on the stream, --reps repetitions after --warmup of
each (median, min - max).  A second loop measures the host wall time each call
takes to ENQUEUE (the stream idle before it, synchronised after it).  Then the
library's own per-kernel event timing (3 calls per case).  One JSON line per
record.  Every output is compared with slices of the input before anything is
timed.  For a comparison over fresh processes run the tool once per case.

  python tools/ragged_decode_bench.py [--cases r,p,q] [--gib 1] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

GIB = 1 << 30


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="r,p,q")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--window", type=int, default=65536)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel pass")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import bench
    import bitshuffle_amd as B
    api = B.api
    if not (torch.cuda.is_available() and B.using_HIP()):
        raise SystemExit("ragged_decode_bench needs the MI355X")

    K, W = args.windows, args.window
    n = int(args.gib * GIB) // 2 // 8 * 8
    x = torch.empty(n, dtype=torch.int16, device="cuda")
    B.synth_fill_dev(x, 1, first=0, seed=12345)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, 2, 0))
    offs = torch.empty(nb, dtype=torch.int64, device="cuda")
    comp = api.compress_lz4_dev(x, offsets=offs)
    rng = torch.Generator().manual_seed(0)
    host_starts = [int(s) | 1 for s in torch.randint(0, n - W, (K,), generator=rng).tolist()]
    host_counts = torch.randint(1, W + 1, (K,), generator=rng).tolist()
    starts = torch.tensor(host_starts, dtype=torch.int64, device="cuda")
    counts = {"r": torch.tensor(host_counts, dtype=torch.int64, device="cuda"),
              "q": torch.full((K,), W, dtype=torch.int64, device="cuda")}

    res = torch.empty(1, dtype=torch.int64, device="cuda")
    status = torch.empty(K, dtype=torch.int64, device="cuda")
    out = torch.empty(K * W, dtype=torch.int16, device="cuda")
    out_offs = torch.empty(K + 1, dtype=torch.int64, device="cuda")
    ws_w = api.decompress_lz4_windows_workspace(comp.numel(), n, 2, K, W)
    ws_r = api.decompress_lz4_ragged_workspace(comp.numel(), n, 2, K, W)

    def ragged(which):
        def fn():
            api.decompress_lz4_ragged_dev(comp, n, torch.int16, starts, counts[which], W, out=out,
                                          out_offsets=out_offs, workspace=ws_r, result=res, status=status,
                                          offsets=offs, sync=False)
        return fn

    def case_p():
        api.decompress_lz4_windows_dev(comp, n, torch.int16, starts, W, out=out.view(K, W), workspace=ws_w,
                                       result=res, status=status, offsets=offs, sync=False)

    table = {"r": ("r_ragged_uniform_counts", ragged("r"), ws_r.numel(), host_counts),
             "p": ("p_windows_padded_to_max", case_p, ws_w.numel(), [W] * K),
             "q": ("q_ragged_equal_counts", ragged("q"), ws_r.numel(), [W] * K)}
    cases = [table[c] for c in args.cases.split(",")]

    for name, fn, _, cs in cases:
        out.zero_()
        fn()
        torch.cuda.synchronize()
        if int(res.item()) != 2 * sum(cs):
            raise SystemExit("%s: result %d" % (name, int(res.item())))
        want = torch.cat([x[s:s + c] for s, c in zip(host_starts, cs)])
        if not torch.equal(out[:want.numel()], want):
            raise SystemExit("%s differs from the input's slices" % name)
        del want

    for _ in range(args.warmup):
        for _, fn, _, _ in cases:
            fn()
    torch.cuda.synchronize()
    ev = {c[0]: [] for c in cases}
    for _ in range(args.reps):
        for name, fn, _, _ in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    enq = {c[0]: [] for c in cases}
    for _ in range(args.reps):
        for name, fn, _, _ in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            enq[name].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    for name, _, wsb, cs in cases:
        ms = [a.elapsed_time(b) for a, b in ev[name]]
        med = statistics.median(ms)
        print(json.dumps({"case": name, "raw_gib": n * 2 / GIB, "stream_bytes": comp.numel(),
                          "windows": K, "max_window_elems": W, "out_mib": round(sum(cs) * 2 / (1 << 20), 3),
                          "workspace_mib": round(wsb / (1 << 20), 3), "reps": args.reps,
                          "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "out_gib_per_s": round(sum(cs) * 2 / GIB / (med / 1e3), 2),
                          "enqueue_ms_median": round(statistics.median(enq[name]), 4),
                          "enqueue_ms_min": round(min(enq[name]), 4),
                          "enqueue_ms_max": round(max(enq[name]), 4)}), flush=True)
    if args.no_kernels:
        return
    for name, fn, _, _ in cases:
        torch.cuda.synchronize()
        B.lib.bshuf_prof_enable(1)
        bench.prof_collect(B.lib)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        k = bench.prof_collect(B.lib)
        B.lib.bshuf_prof_enable(0)
        print(json.dumps({"case": name, "kernel_ms_per_call": {
            kn: round(ms / 3, 4) for kn, (cnt, ms) in sorted(k.items())}}), flush=True)


if __name__ == "__main__":
    main()

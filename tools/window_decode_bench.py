#!/usr/bin/env python3
"""Window decode against the host-planned range decode, device-resident.

The stream and the windows of tools/range_decode_bench.py's case (d): one G1
int16 stream (synth_fill_dev, default block size, --gib of raw data) with its
block index, and 4096 windows of 65,536 elements at odd starts.

  d  decompress_lz4_ranges_dev of the 4096 (start, 65536) ranges: planned on
     the CPU from a host list, the piece table uploaded
  e  decompress_lz4_windows_dev of the same starts held in a device tensor

Both with a caller workspace, output, result and the index supplied.  The two
are timed in ONE loop, alternating d, e, d, e, ..., each call between two device
events on the stream, --reps repetitions after --warmup of each (median, min -
max).  A second loop measures the host wall time each call takes to ENQUEUE
(the stream idle before it, synchronised after it).  Then the library's own
per-kernel event timing (3 calls per case) gives each kernel's ms per call.
One JSON line per record.  Both outputs are compared with slices of the input
before anything is timed.

  python tools/window_decode_bench.py [--gib 1] [--reps 20] [--warmup 3]
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
        raise SystemExit("window_decode_bench needs the MI355X")

    K, W = args.windows, args.window
    n = int(args.gib * GIB) // 2 // 8 * 8
    x = torch.empty(n, dtype=torch.int16, device="cuda")
    B.synth_fill_dev(x, 1, first=0, seed=12345)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, 2, 0))
    offs = torch.empty(nb, dtype=torch.int64, device="cuda")
    comp = api.compress_lz4_dev(x, offsets=offs)
    rng = torch.Generator().manual_seed(0)
    host_starts = [int(s) | 1 for s in torch.randint(0, n - W, (K,), generator=rng).tolist()]
    rs = [(s, W) for s in host_starts]
    starts = torch.tensor(host_starts, dtype=torch.int64, device="cuda")

    res = torch.empty(1, dtype=torch.int64, device="cuda")
    out_d = torch.empty(K * W, dtype=torch.int16, device="cuda")
    out_e = torch.empty((K, W), dtype=torch.int16, device="cuda")
    ws_d = api.decompress_lz4_ranges_workspace(comp.numel(), n, 2, rs)
    ws_e = api.decompress_lz4_windows_workspace(comp.numel(), n, 2, K, W)

    def case_d():
        api.decompress_lz4_ranges_dev(comp, n, torch.int16, rs, out=out_d, workspace=ws_d, result=res,
                                      offsets=offs, sync=False)

    def case_e():
        api.decompress_lz4_windows_dev(comp, n, torch.int16, starts, W, out=out_e, workspace=ws_e,
                                       result=res, offsets=offs, sync=False)

    want = torch.cat([x[s:s + W] for s in host_starts])
    for fn, out in ((case_d, out_d), (case_e, out_e)):
        out.zero_()
        fn()
        torch.cuda.synchronize()
        if int(res.item()) != 2 * K * W or not torch.equal(out.reshape(-1), want):
            raise SystemExit("%s differs from the input's slices" % fn.__name__)
    del want
    cases = [("d_ranges_host_planned", case_d, ws_d.numel()), ("e_windows_device_starts", case_e, ws_e.numel())]

    for _ in range(args.warmup):
        for _, fn, _ in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _, _ in cases}
    for _ in range(args.reps):
        for name, fn, _ in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    enq = {name: [] for name, _, _ in cases}
    for _ in range(args.reps):
        for name, fn, _ in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            enq[name].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    for name, _, wsb in cases:
        ms = [a.elapsed_time(b) for a, b in ev[name]]
        med = statistics.median(ms)
        print(json.dumps({"case": name, "raw_gib": n * 2 / GIB, "stream_bytes": comp.numel(),
                          "windows": K, "window_elems": W, "out_mib": round(K * W * 2 / (1 << 20), 3),
                          "workspace_mib": round(wsb / (1 << 20), 3), "reps": args.reps,
                          "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "out_gib_per_s": round(K * W * 2 / GIB / (med / 1e3), 2),
                          "enqueue_ms_median": round(statistics.median(enq[name]), 4),
                          "enqueue_ms_min": round(min(enq[name]), 4),
                          "enqueue_ms_max": round(max(enq[name]), 4)}), flush=True)
    if args.no_kernels:
        return
    for name, fn, _ in cases:
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

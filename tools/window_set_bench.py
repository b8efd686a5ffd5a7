#!/usr/bin/env python3
"""Window decode over a set of streams against one window call per stream.

The set: --streams G1 int16 streams of --mib MiB raw data each (synth_fill_dev,
one compress_lz4_batch_dev, default block size) with their block indexes.  The
windows: --windows windows of --window elements at odd starts and random ids,
both in device tensors.

  s  decompress_lz4_windows_set_dev: one call, ids and starts stay on the device
  l  what a caller does without it: ids and starts read back, grouped by stream
     on the host, one decompress_lz4_windows_dev per stream (indexes supplied,
     one workspace sized for the largest group), rows scattered back

Both write the same (K, window) output, compared with slices of the inputs
before anything is timed.  Timed in ONE loop, alternating s, l, s, l, ...: device
events on the stream around each, --reps repetitions after --warmup (median,
min - max); a second loop measures the host wall time each takes to return, the
stream idle before it (for s: the time to enqueue; l waits for its own read
back).  Then the one-off set build, indexes supplied and rebuilt: wall time
from an idle stream to a synchronised one, and its device time.  One JSON line
per record.

  python tools/window_set_bench.py [--streams 64] [--mib 16] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

MIB = 1 << 20


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--mib", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--window", type=int, default=65536)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import bitshuffle_amd as B
    api = B.api
    if not (torch.cuda.is_available() and B.using_HIP()):
        raise SystemExit("window_set_bench needs the MI355X")

    S, K, W = args.streams, args.windows, args.window
    n = int(args.mib * MIB) // 2 // 8 * 8
    xs = [torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(S)]
    for i, x in enumerate(xs):
        B.synth_fill_dev(x, 1, first=i * n, seed=12345)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, 2, 0))
    offs = torch.empty(S * nb, dtype=torch.int64, device="cuda")
    comps = api.compress_lz4_batch_dev(xs, offsets=offs)
    comps = [c.clone() for c in comps]          # each stream in a buffer of its own length
    idx = [offs[i * nb:(i + 1) * nb] for i in range(S)]
    g = torch.Generator(device="cuda").manual_seed(0)
    ids = torch.randint(0, S, (K,), generator=g, device="cuda", dtype=torch.int64)
    starts = torch.randint(0, n - W, (K,), generator=g, device="cuda", dtype=torch.int64) | 1

    sset = api.lz4_stream_set_dev(comps, [n] * S, 2, offsets=idx)
    res = torch.empty(1, dtype=torch.int64, device="cuda")
    out_s = torch.empty((K, W), dtype=torch.int16, device="cuda")
    out_l = torch.empty((K, W), dtype=torch.int16, device="cuda")
    tmp_l = torch.empty((K, W), dtype=torch.int16, device="cuda")
    ws_s = api.decompress_lz4_windows_set_workspace(sset, K, W)
    ws_l = api.decompress_lz4_windows_workspace(max(c.numel() for c in comps), n, 2, K, W)
    ncalls = [0]

    def case_s():
        api.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, W, out=out_s, workspace=ws_s,
                                           result=res, sync=False)

    def case_l():
        hid = ids.cpu().numpy()
        hst = starts.cpu().numpy()
        order = np.argsort(hid, kind="stable")
        counts = np.bincount(hid, minlength=S)
        sorted_starts = torch.from_numpy(hst[order]).cuda()
        at = 0
        ncalls[0] = 0
        for s in range(S):
            k = int(counts[s])
            if k == 0:
                continue
            api.decompress_lz4_windows_dev(comps[s], n, torch.int16, sorted_starts[at:at + k], W,
                                           out=tmp_l[at:at + k], workspace=ws_l, result=res, offsets=idx[s],
                                           sync=False)
            at += k
            ncalls[0] += 1
        out_l.index_copy_(0, torch.from_numpy(order).cuda(), tmp_l)

    hid, hst = ids.cpu().tolist(), starts.cpu().tolist()
    want = torch.stack([xs[i][s:s + W] for i, s in zip(hid, hst)])
    for fn, out in ((case_s, out_s), (case_l, out_l)):
        out.zero_()
        fn()
        torch.cuda.synchronize()
        if not torch.equal(out, want):
            raise SystemExit("%s differs from the inputs' slices" % fn.__name__)
    del want
    cases = [("s_windows_set", case_s, ws_s.numel()), ("l_loop_per_stream", case_l, ws_l.numel())]

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
        print(json.dumps({"case": name, "streams": S, "raw_mib_per_stream": n * 2 / MIB,
                          "stream_bytes": sum(c.numel() for c in comps), "windows": K, "window_elems": W,
                          "out_mib": round(K * W * 2 / MIB, 3), "workspace_mib": round(wsb / MIB, 3),
                          "window_calls": 1 if name[0] == "s" else ncalls[0], "reps": args.reps,
                          "event_ms": stats(ms), "host_ms_to_return": stats(enq[name])}), flush=True)

    # the one-off set build
    for name, offsets in (("set_build_indexes_supplied", idx), ("set_build_indexes_rebuilt", None)):
        wall, dev = [], []
        for _ in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            built = api.lz4_stream_set_dev(comps, [n] * S, 2, offsets=offsets)
            b.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(a.elapsed_time(b))
        assert built.status.cpu().tolist() == [0] * S
        print(json.dumps({"case": name, "streams": S, "set_bytes": built.table.numel(),
                          "wall_ms": stats(wall[args.warmup:]), "event_ms": stats(dev[args.warmup:])}),
              flush=True)


if __name__ == "__main__":
    main()

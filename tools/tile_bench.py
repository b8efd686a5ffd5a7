#!/usr/bin/env python3
"""Tile decode over a set of streams against the window call a caller expands it to.

Case A, images: --streams frames of 2048 x 2048 int16 G1 (synth_fill_dev, one
compress_lz4_batch_dev, default block size, indexes supplied), --tiles tiles of
256 x 256 at random corners of random frames, ids and corners drawn on the device.
Case B, wide rows: float32 G2 frames of 512 x 16384, the same tiles: every row
is eight blocks from the next, both calls decode the same blocks.

  t  decompress_lz4_tiles_set_dev: one call
  w  what a caller does without it: starts[i] + r * pitch and the ids repeated,
     made with torch ops on the device (timed inside w), then one
     decompress_lz4_windows_set_dev over the K * rows windows of cols elements

Both write the same (K, rows, cols) output, compared with slices of the inputs
before anything is timed.  Timed in ONE loop, alternating t, w, t, w, ...: device
events on the stream around each, --reps repetitions after --warmup (median, min
- max); a second loop measures the host wall time each takes to return from an
idle stream (the time to enqueue).  Then, per case, t with the gather's lanes
per row forced (bshuf_set_variant 1 << 22, 1 << 23, both: 16, 64, 256), in one
alternating loop with the default, and one pass of each of t and w, and of t
at each forced lane count, under the library's per-kernel event timing.  The first record is the clock state as
rocm-smi reports it before and after.  One JSON line per record.

  python tools/tile_bench.py [--streams 64] [--tiles 1024] [--reps 20] [--warmup 3] [--case A|B|AB]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

MIB = 1 << 20
LANES = {16: 1 << 22, 64: 1 << 23, 256: (1 << 22) | (1 << 23)}   # kTileLanes16 / 64 / 256 (launch.h)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True,
                             timeout=30).stdout
        keep = [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("clk" in ln or "Perf" in ln)]
        return keep or "rocm-smi printed no clocks"
    except Exception as e:  # noqa: BLE001
        return "not read: %s" % e


def timed(torch, cases, reps, warmup):
    """cases: (name, fn); one alternating loop of device events, one of host times."""
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cases}
    for _ in range(reps):
        for name, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    enq = {name: [] for name, _ in cases}
    for _ in range(reps):
        for name, fn in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            enq[name].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return ({name: stats([a.elapsed_time(b) for a, b in ev[name]]) for name, _ in cases},
            {name: stats(enq[name]) for name, _ in cases})


def run_case(args, torch, B, bench, label, dtype, gen, height, pitch):
    api = B.api
    S, K, rows, cols = args.streams if label == "A" else max(args.streams // 4, 1), args.tiles, 256, 256
    es = torch.empty(0, dtype=dtype).element_size()
    n = height * pitch
    xs = [torch.empty(n, dtype=dtype, device="cuda") for _ in range(S)]
    for i, x in enumerate(xs):
        B.synth_fill_dev(x, gen, first=i * n, seed=12345)
    bs = B.default_block_size(es)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, es, 0))
    offs = torch.empty(S * nb, dtype=torch.int64, device="cuda")
    comps = [c.clone() for c in api.compress_lz4_batch_dev(xs, offsets=offs)]
    idx = [offs[i * nb:(i + 1) * nb] for i in range(S)]
    g = torch.Generator(device="cuda").manual_seed(0)
    ids = torch.randint(0, S, (K,), generator=g, device="cuda", dtype=torch.int64)
    ys = torch.randint(0, height - rows + 1, (K,), generator=g, device="cuda", dtype=torch.int64)
    xc = torch.randint(0, pitch - cols + 1, (K,), generator=g, device="cuda", dtype=torch.int64)
    starts = ys * pitch + xc
    sset = api.lz4_stream_set_dev(comps, [n] * S, es, offsets=idx)
    res = torch.empty(1, dtype=torch.int64, device="cuda")
    out_t = torch.empty((K, rows, cols), dtype=dtype, device="cuda")
    out_w = torch.empty((K, rows, cols), dtype=dtype, device="cuda")
    ws_t = api.decompress_lz4_tiles_set_workspace(sset, K, rows, cols, pitch)
    ws_w = api.decompress_lz4_windows_set_workspace(sset, K * rows, cols)
    step = torch.arange(rows, device="cuda", dtype=torch.int64) * pitch

    def case_t():
        api.decompress_lz4_tiles_set_dev(sset, dtype, ids, starts, rows, cols, pitch, out=out_t, workspace=ws_t,
                                         result=res, sync=False)

    def case_w():
        wst = (starts[:, None] + step[None, :]).reshape(-1)
        wid = ids.repeat_interleave(rows)
        api.decompress_lz4_windows_set_dev(sset, dtype, wid, wst, cols, out=out_w.view(K * rows, cols),
                                           workspace=ws_w, result=res, sync=False)

    hid, hy, hx = ids.cpu().tolist(), ys.cpu().tolist(), xc.cpu().tolist()
    want = torch.stack([xs[i].view(height, pitch)[y:y + rows, x:x + cols] for i, y, x in zip(hid, hy, hx)])
    total = K * rows * cols * es
    for fn, out in ((case_t, out_t), (case_w, out_w)):
        out.zero_()
        fn()
        torch.cuda.synchronize()
        if int(res.item()) != total or not torch.equal(out, want):
            raise SystemExit("case %s: %s differs from the inputs' slices" % (label, fn.__name__))

    def forced(lanes):
        def f():
            if B.lib.bshuf_set_variant(LANES[lanes]) != 0:
                raise SystemExit("bshuf_set_variant refuses the value for %d lanes per row" % lanes)
            case_t()
            if B.lib.bshuf_set_variant(0) != 0:
                raise SystemExit("bshuf_set_variant refuses 0")
        return f
    # byte-identical: checked before they are timed
    for lanes in LANES:
        out_t.zero_()
        forced(lanes)()
        torch.cuda.synchronize()
        if not torch.equal(out_t, want):
            raise SystemExit("case %s: %d lanes per row differ" % (label, lanes))
    del want

    shape = {"rows": rows, "cols": cols, "pitch": pitch, "elem_size": es, "block_elems": bs,
             "row_bytes": cols * es}
    base = {"case": label, "streams": S, "raw_mib_per_stream": n * es / MIB,
            "stream_bytes": sum(c.numel() for c in comps), "tiles": K, "shape": shape,
            "out_mib": round(total / MIB, 3), "reps": args.reps}
    ev, enq = timed(torch, [("t_tiles_set", case_t), ("w_windows_expanded", case_w)], args.reps, args.warmup)
    for name, wsb in (("t_tiles_set", ws_t.numel()), ("w_windows_expanded", ws_w.numel())):
        print(json.dumps(dict(base, call=name, workspace_mib=round(wsb / MIB, 3), event_ms=ev[name],
                              host_ms_to_return=enq[name])), flush=True)
    print(json.dumps(dict(base, call="t_over_w", ratio_of_medians=round(
        ev["t_tiles_set"]["median"] / ev["w_windows_expanded"]["median"], 4))), flush=True)

    ev, _ = timed(torch, [("default", case_t), ("lanes_16", forced(16)), ("lanes_64", forced(64)),
                          ("lanes_256", forced(256))], args.reps, args.warmup)
    print(json.dumps(dict(base, call="t_gather_lanes_per_row", event_ms=ev)), flush=True)

    def kernels(fn):
        torch.cuda.synchronize()
        B.lib.bshuf_prof_enable(1)
        bench.prof_collect(B.lib)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        k = bench.prof_collect(B.lib)
        B.lib.bshuf_prof_enable(0)
        return {kn: round(ms / 5, 4) for kn, (cnt, ms) in sorted(k.items())}
    for name, fn in (("t_tiles_set", case_t), ("w_windows_expanded", case_w)):
        print(json.dumps(dict(base, call=name, kernel_ms_per_call=kernels(fn))), flush=True)
    # the gather alone, per forced lane count
    print(json.dumps(dict(base, call="t_gather_kernel_ms", kernel_ms_per_call={
        "lanes_%d" % lanes: kernels(forced(lanes))["k_tile_set_gather"] for lanes in LANES})), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default="AB")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch

    import bench
    import bitshuffle_amd as B
    if not (torch.cuda.is_available() and B.using_HIP()):
        raise SystemExit("tile_bench needs the MI355X")
    print(json.dumps({"clocks_before": clocks()}), flush=True)
    if "A" in args.case:
        run_case(args, torch, B, bench, "A", torch.int16, 1, 2048, 2048)
    if "B" in args.case:
        run_case(args, torch, B, bench, "B", torch.float32, 2, 512, 16384)
    print(json.dumps({"clocks_after": clocks()}), flush=True)


if __name__ == "__main__":
    main()

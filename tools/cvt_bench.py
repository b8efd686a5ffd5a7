#!/usr/bin/env python3
"""Decode to float, fused against the two steps it replaces, and the plain calls alone.

Shape T, tiles: --streams frames of 2048 x 2048 int16 G1 (synth_fill_dev, one
compress_lz4_batch_dev, default block size, indexes supplied), --tiles crops of
256 x 256 at random corners of random frames, over a stream set.
Shape W, windows: --streams streams of 16 MiB of int16 G1, --windows windows of
128 KiB (65536 elements) at odd starts in random streams, over a stream set.
Ids and starts are drawn on the device.  For each shape and each of float32 and
bfloat16:

  plain     decompress_lz4_tiles_set_dev / decompress_lz4_windows_set_dev
  fused     the same call with out_dtype=, scale=1, offset=0: one call, one buffer
  two_step  the plain call, then ONE torch cast kernel, out.to(out_dtype)

fused and two_step give the same values (torch.equal, checked before anything
is timed; plain is checked against slices of the inputs).  Timing: --rounds
rounds, each ONE loop that alternates plain, fused, two_step, ... --reps times
after --warmup, device events on the stream around each case.  A case's figure
is the median over the rounds of the round's median; its run-to-run spread is
the range of the rounds' medians.  `speedup_claimable`: the fused median is
below the two-step median by more than the larger of the two spreads.  Then one
pass of fused and two_step under the library's per-kernel event timing.

--plain-only times the plain calls alone, which also runs on a checkout
without the converting entries; --root names that checkout (default: this
file's), so that two commits can be timed by alternating runs of this tool.
With --lanes (shape T): the fused call with the tile gather's lanes per row
forced to 16 / 64 / 256 (bshuf_set_variant), at crops of 256 x 256 int16 to
float32 (512-byte source rows) and of 256 x 512 (1024-byte source rows).
The first and last records are the clocks as rocm-smi reports them.  One JSON
line per record.

  python tools/cvt_bench.py [--shape TW] [--rounds 5] [--reps 20] [--warmup 3] [--plain-only] [--lanes]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

MIB = 1 << 20
LANES = {16: 1 << 22, 64: 1 << 23, 256: (1 << 22) | (1 << 23)}   # kTileLanes16 / 64 / 256 (launch.h)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True,
                             timeout=30).stdout
        keep = [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("clk" in ln or "Perf" in ln)]
        return keep or "rocm-smi printed no clocks"
    except Exception as e:  # noqa: BLE001
        return "not read: %s" % e


def rounds_of(torch, cases, rounds, reps, warmup):
    """cases: (name, fn).  Per case: the rounds' medians (ms)."""
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    med = {name: [] for name, _ in cases}
    for _ in range(rounds):
        ev = {name: [] for name, _ in cases}
        for _ in range(reps):
            for name, fn in cases:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        for name, _ in cases:
            med[name].append(statistics.median(a.elapsed_time(b) for a, b in ev[name]))
    return med


def figure(ms):
    return {"median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "round_medians_ms": [round(m, 4) for m in ms]}


def make_set(torch, B, S, n):
    """S streams of n int16 G1 elements; returns (inputs, set)."""
    api = B.api
    xs = [torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(S)]
    for i, x in enumerate(xs):
        B.synth_fill_dev(x, 1, first=i * n, seed=12345)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, 2, 0))
    offs = torch.empty(S * nb, dtype=torch.int64, device="cuda")
    comps = [c.clone() for c in api.compress_lz4_batch_dev(xs, offsets=offs)]
    idx = [offs[i * nb:(i + 1) * nb] for i in range(S)]
    return xs, api.lz4_stream_set_dev(comps, [n] * S, 2, offsets=idx)


def kernels(torch, B, bench, fn):
    torch.cuda.synchronize()
    B.lib.bshuf_prof_enable(1)
    bench.prof_collect(B.lib)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    k = bench.prof_collect(B.lib)
    B.lib.bshuf_prof_enable(0)
    return {kn: round(ms / 5, 4) for kn, (cnt, ms) in sorted(k.items())}


def run_shape(args, torch, B, bench, label):
    api = B.api
    S = args.streams
    g = torch.Generator(device="cuda").manual_seed(0)
    res = torch.empty(1, dtype=torch.int64, device="cuda")
    if label == "T":
        height = pitch = 2048
        K, rows, cols = args.tiles, 256, args.cols
        xs, sset = make_set(torch, B, S, height * pitch)
        ids = torch.randint(0, S, (K,), generator=g, device="cuda", dtype=torch.int64)
        ys = torch.randint(0, height - rows + 1, (K,), generator=g, device="cuda", dtype=torch.int64)
        xc = torch.randint(0, pitch - cols + 1, (K,), generator=g, device="cuda", dtype=torch.int64)
        starts = ys * pitch + xc
        ws = api.decompress_lz4_tiles_set_workspace(sset, K, rows, cols, pitch)
        shape = (K, rows, cols)
        want = torch.stack([xs[i].view(height, pitch)[y:y + rows, x:x + cols]
                            for i, y, x in zip(ids.cpu().tolist(), ys.cpu().tolist(), xc.cpu().tolist())])

        def call(out, **kw):
            api.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, starts, rows, cols, pitch, out=out,
                                             workspace=ws, result=res, sync=False, **kw)
        what = {"shape": "T", "streams": S, "tiles": K, "rows": rows, "cols": cols, "pitch": pitch}
    else:
        n, K, window = 8 * MIB, args.windows, 65536
        xs, sset = make_set(torch, B, S, n)
        ids = torch.randint(0, S, (K,), generator=g, device="cuda", dtype=torch.int64)
        starts = torch.randint(0, (n - window) // 2, (K,), generator=g, device="cuda", dtype=torch.int64) * 2 + 1
        ws = api.decompress_lz4_windows_set_workspace(sset, K, window)
        shape = (K, window)
        want = torch.stack([xs[i][s:s + window] for i, s in zip(ids.cpu().tolist(), starts.cpu().tolist())])

        def call(out, **kw):
            api.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, window, out=out, workspace=ws,
                                               result=res, sync=False, **kw)
        what = {"shape": "W", "streams": S, "windows": K, "window": window}
    del xs
    total = want.numel() * 2
    what.update(elem_size=2, source_mib=round(total / MIB, 1), workspace_mib=round(ws.numel() / MIB, 1),
                rounds=args.rounds, reps=args.reps)
    out_p = torch.empty(shape, dtype=torch.int16, device="cuda")

    def plain():
        call(out_p)
    out_p.zero_()
    plain()
    torch.cuda.synchronize()
    if int(res.item()) != total or not torch.equal(out_p, want):
        raise SystemExit("shape %s: the plain call differs from the inputs' slices" % label)
    if args.plain_only:
        med = rounds_of(torch, [("plain", plain)], args.rounds, args.reps, args.warmup)
        print(json.dumps(dict(what, call="plain", **figure(med["plain"]))), flush=True)
        return
    for dt in (torch.float32, torch.bfloat16):
        out_f = torch.empty(shape, dtype=dt, device="cuda")
        kw = dict(out_dtype=dt, scale=1.0, offset=0.0)
        keep = []

        def fused():
            call(out_f, **kw)

        def two_step():
            call(out_p)
            keep[:] = [out_p.to(dt)]
        out_f.zero_()
        fused()
        two_step()
        torch.cuda.synchronize()
        if int(res.item()) != total or not torch.equal(out_f, keep[0]) or not torch.equal(out_f, want.to(dt)):
            raise SystemExit("shape %s: fused, two-step and the inputs' slices differ (%s)" % (label, dt))
        rec = dict(what, out_dtype=str(dt), out_mib=round(out_f.numel() * out_f.element_size() / MIB, 1))
        if args.lanes and label == "T":
            def forced(lanes):
                def f():
                    if B.lib.bshuf_set_variant(LANES[lanes]) != 0:
                        raise SystemExit("bshuf_set_variant refuses the value for %d lanes per row" % lanes)
                    fused()
                    if B.lib.bshuf_set_variant(0) != 0:
                        raise SystemExit("bshuf_set_variant refuses 0")
                return f
            for lanes in LANES:
                out_f.zero_()
                forced(lanes)()
                torch.cuda.synchronize()
                if not torch.equal(out_f, keep[0]):
                    raise SystemExit("%d lanes per row differ" % lanes)
            print(json.dumps(dict(rec, call="fused_gather_kernel_ms", source_row_bytes=cols * 2, kernel_ms_per_call={
                "lanes_%d" % lanes: kernels(torch, B, bench, forced(lanes))["k_tile_set_gather"]
                for lanes in LANES})), flush=True)
            continue
        med = rounds_of(torch, [("plain", plain), ("fused", fused), ("two_step", two_step)], args.rounds,
                        args.reps, args.warmup)
        fig = {name: figure(ms) for name, ms in med.items()}
        for name in ("plain", "fused", "two_step"):
            print(json.dumps(dict(rec, call=name, **fig[name])), flush=True)
        gain = fig["two_step"]["median_ms"] - fig["fused"]["median_ms"]
        margin = max(fig["two_step"]["spread_ms"], fig["fused"]["spread_ms"])
        print(json.dumps(dict(rec, call="fused_vs_two_step", two_step_minus_fused_ms=round(gain, 4),
                              larger_spread_ms=margin, speedup_claimable=bool(gain > margin))), flush=True)
        for name, fn in (("fused", fused), ("two_step", two_step)):
            print(json.dumps(dict(rec, call=name, kernel_ms_per_call=kernels(torch, B, bench, fn))), flush=True)
        del keep[:]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="TW")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--lanes", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import bench
    import bitshuffle_amd as B
    if not (torch.cuda.is_available() and B.using_HIP()):
        raise SystemExit("cvt_bench needs the MI355X")
    print(json.dumps({"clocks_before": clocks(), "package": os.path.dirname(B.__file__)}), flush=True)
    for label in args.shape:
        run_shape(args, torch, B, bench, label)
        torch.cuda.empty_cache()
    print(json.dumps({"clocks_after": clocks()}), flush=True)


if __name__ == "__main__":
    main()

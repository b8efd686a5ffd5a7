#!/usr/bin/env python3
"""Range decode against the whole decode, device-resident.

One G1 int16 stream (synth_fill_dev, default block size, --gib of raw data)
stays on the device with its block index.  Timed, each with device events on
the stream after a warm-up, median of --reps repetitions (min / max as the
spread):

  a  decompress_lz4_dev of the whole stream with offsets, then a slice of 1/8
     of the array (what a caller without the range decode does)
  b  one block-aligned range of 1/8 of the array, with offsets
  c  the same range, the index rebuilt by the call
  d  4096 random ranges of 65,536 elements, unaligned, with offsets

One JSON line per case.  Every case's output is compared with the whole
decode's before it is timed.  After the timed loops, the library's own
per-kernel event timing (3 calls per case) gives each kernel's ms per call; it
is not on during the timed loops.

  python tools/range_decode_bench.py [--gib 1] [--reps 20] [--warmup 3] [--root DIR]

--root DIR imports the package from another checkout (a checkout without the
range decode runs case a only).
"""
import argparse
import json
import os
import statistics
import sys

GIB = 1 << 30


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel pass")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import bench
    import bitshuffle_amd as B
    api = B.api
    if not (torch.cuda.is_available() and B.using_HIP()):
        raise SystemExit("range_decode_bench needs the MI355X")
    have_ranges = hasattr(api, "decompress_lz4_ranges_dev")

    n = int(args.gib * GIB) // 2 // 8 * 8
    x = torch.empty(n, dtype=torch.int16, device="cuda")
    B.synth_fill_dev(x, 1, first=0, seed=12345)
    nb = int(B.lib.bshuf_lz4_dev_nblocks(n, 2, 0))
    offs = torch.empty(nb, dtype=torch.int64, device="cuda")
    comp = api.compress_lz4_dev(x, offsets=offs)
    bs = B.default_block_size(2)
    # 1/8 of the array on block boundaries, from block nb/2 on
    start, count = (nb // 2) * bs, (nb // 8) * bs
    rng = torch.Generator().manual_seed(0)
    rs = [(int(s) | 1, 65536) for s in torch.randint(0, n - 65536, (4096,), generator=rng).tolist()]

    whole = torch.empty(n, dtype=torch.int16, device="cuda")
    res = torch.empty(1, dtype=torch.int64, device="cuda")
    ws_whole = api.decompress_lz4_workspace(comp.numel(), n, 2)
    keep = torch.empty(count, dtype=torch.int16, device="cuda")

    def case_a():
        api.decompress_lz4_dev(comp, (n,), torch.int16, out=whole, workspace=ws_whole, result=res,
                               offsets=offs, sync=False)
        keep.copy_(whole[start:start + count])

    case_a()
    torch.cuda.synchronize()
    if int(res.item()) != comp.numel() or not torch.equal(whole, x):
        raise SystemExit("the whole decode does not return the input")
    cases = [("a_whole_decode_then_slice", case_a, count)]

    if have_ranges:
        out_b = torch.empty(count, dtype=torch.int16, device="cuda")
        ws_b = api.decompress_lz4_ranges_workspace(comp.numel(), n, 2, [(start, count)])
        out_d = torch.empty(65536 * len(rs), dtype=torch.int16, device="cuda")
        ws_d = api.decompress_lz4_ranges_workspace(comp.numel(), n, 2, rs)

        def ranges(r, out, ws, o):
            api.decompress_lz4_ranges_dev(comp, n, torch.int16, r, out=out, workspace=ws, result=res,
                                          offsets=o, sync=False)

        def case_b():
            ranges([(start, count)], out_b, ws_b, offs)

        def case_c():
            ranges([(start, count)], out_b, ws_b, None)

        def case_d():
            ranges(rs, out_d, ws_d, offs)

        for fn in (case_b, case_c):
            out_b.zero_()
            fn()
            torch.cuda.synchronize()
            if int(res.item()) != 2 * count or not torch.equal(out_b, x[start:start + count]):
                raise SystemExit("%s differs from the whole decode" % fn.__name__)
        case_d()
        torch.cuda.synchronize()
        want = torch.cat([x[s:s + c] for s, c in rs])
        if int(res.item()) != 2 * out_d.numel() or not torch.equal(out_d, want):
            raise SystemExit("case_d differs from the whole decode")
        del want
        cases += [("b_aligned_eighth_with_offsets", case_b, count),
                  ("c_aligned_eighth_index_rebuilt", case_c, count),
                  ("d_4096_unaligned_ranges_with_offsets", case_d, out_d.numel())]

    for name, fn, elems in cases:
        med, lo, hi = timed(torch, fn, args.reps, args.warmup)
        print(json.dumps({"case": name, "raw_gib": n * 2 / GIB, "stream_bytes": comp.numel(),
                          "out_mib": round(elems * 2 / (1 << 20), 3), "reps": args.reps,
                          "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "out_gib_per_s": round(elems * 2 / GIB / (med / 1e3), 2)}), flush=True)
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

"""Phase split of k_lz4_encode from the diagnostic build (BSHUF_DIAG stamps).
Usage: python tools/diag_encode.py [GiB] [gen] [elem_size] [variant]   (runs on the GPU box;
variant 16777216 = static block assignment, 67108864 = no stealing between
ticket shards, 3072000 = round 5's emission).  BSHUF_DIAG_SKEW=s: noise in the blocks = s (mod 8), zeros
elsewhere.  Ends with the per-shard finish table of the call's parse launches."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["BSHUF_LIB"] = os.path.join(ROOT, "bitshuffle_amd", "libbitshuffle_mi355x_diag.so")
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bitshuffle_amd as B  # noqa: E402
from bitshuffle_amd import api  # noqa: E402

def skew(x, s):
    """Noise in the default-size (8 KiB) blocks whose index is s (mod 8), zeros elsewhere."""
    b = x.view(torch.uint8)
    rows = b[: b.numel() // 8192 * 8192].view(-1, 8192)
    rows.zero_()
    rows[s::8] = torch.randint(0, 256, rows[s::8].shape, dtype=torch.uint8, device=x.device)


def shard_table(read, what):
    """Per launch and ticket shard (the diag build's ShardDiag): the last exit of
    the shard's waves after the launch's first start, in us of the 100 MHz
    s_memrealtime, and the blocks its waves took from their own shard and from others."""
    S, W, SLOTS = 8, 5, 16
    buf = (ctypes.c_ulonglong * (SLOTS * S * W))()
    n = read(buf)
    print("%s: %d launches since the last read; exit of each home shard's last wave, us after the "
          "launch's first start" % (what, n))
    for slot in range(min(n, SLOTS)):
        rows = [[buf[(slot * S + c) * W + i] for i in range(W)] for c in range(S)]
        rows = [r if r[0] != 2 ** 64 - 1 else None for r in rows]
        live = [r for r in rows if r]
        if not live:
            continue
        t0 = min(r[0] for r in live)
        ex = [(r[1] - t0) / 100.0 if r else float("nan") for r in rows]
        fin = [e for e in ex if e == e]
        print("  launch %2d  exit us: %s  spread %.1f us (%.1f%% of %.1f)  last shard %d" % (
            slot, " ".join("%7.1f" % e for e in ex), max(fin) - min(fin),
            100.0 * (max(fin) - min(fin)) / max(fin), max(fin), ex.index(max(fin))))
        print("             own blocks: %s" % " ".join("%7d" % (r[2] if r else 0) for r in rows))
        print("             stolen:     %s   (thieves: %s)" % (
            " ".join("%7d" % (r[3] if r else 0) for r in rows),
            " ".join("%d" % (r[4] if r else 0) for r in rows)))


gib = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
gen = int(sys.argv[2]) if len(sys.argv) > 2 else 1
es = int(sys.argv[3]) if len(sys.argv) > 3 else 0  # element size override (the same bytes)
n = int(gib * (1 << 30)) // (2 if gen == 1 else 4)
x = torch.empty(n, dtype=torch.int16 if gen == 1 else torch.float32, device="cuda")
B.synth_fill_dev(x, gen)
if os.environ.get("BSHUF_DIAG_SKEW"):
    skew(x, int(os.environ["BSHUF_DIAG_SKEW"]))
if es:
    x = x.view(torch.uint8)[: (x.numel() * x.element_size() // es) * es]
if len(sys.argv) > 4:
    assert B.lib.bshuf_set_variant(int(sys.argv[4])) == 0
rd = B.lib.bshuf_diag_read
rd.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_ulonglong * 32)()
c = api.compress_lz4_dev(x, elem_size=es or None)
torch.cuda.synchronize()
rd(buf)  # reset after warm-up
rds = B.lib.bshuf_diag_read_shards
rds.argtypes = [ctypes.c_void_p]
rds((ctypes.c_ulonglong * 640)())
B.lib.bshuf_prof_enable(1)
c = api.compress_lz4_dev(x, elem_size=es or None)
torch.cuda.synchronize()
rd(buf)
import bench  # noqa: E402
prof = bench.prof_collect(B.lib)
v = list(buf)
names = ["search", "catch+count", "(unused)", "seq-record", "retest", "last"]
cnt = ["matches", "windows", "collision_windows", "retest_hits", "blocks", "literal_bytes",
       "searches"]
blocks = max(v[12] or v[22], 1)  # the asm parse does not count blocks: the waves' sum
tot = sum(v[:6])
print("blocks", blocks, "ratio", x.numel() * x.element_size() / c.numel())
for i, nm in enumerate(names):
    print("%-12s %8.0f cyc/block  %5.1f%%" % (nm, v[i] / blocks, 100.0 * v[i] / max(tot, 1)))
print("parse cycles/block %.0f" % (tot / blocks))
kn = ["zero+transpose", "parse", "emit+copy-out", "loop/other"]
ktot = sum(v[16:20])
for i, nm in enumerate(kn):
    print("kernel %-15s %8.0f cyc/block  %5.1f%%" % (nm, v[16 + i] / blocks, 100.0 * v[16 + i] / max(ktot, 1)))
# the emission's sub-phases (each stamp drains the LDS queue, so they add up
# to more than the product build's emission) and events
en = ["desc+prefix", "token/len/offset", "lane runs", "wave runs"]
for i, nm in enumerate(en):
    print("emit %-17s %8.0f cyc/block  %5.1f%% of emit+copy-out" % (nm, v[24 + i] / blocks, 100.0 * v[24 + i] / max(v[18], 1)))
ec = ["runs_per_lane", "runs_by_wave", "wave_copy_steps", "len_run_steps"]
for i, nm in enumerate(ec):
    print("%-18s %8.2f per block" % (nm, v[28 + i] / blocks))
for i, nm in enumerate(cnt):
    print("%-18s %8.2f per block" % (nm, v[8 + i] / blocks))
# blocks per wave over the call's parse launches: equal under the static
# schedule, spread under tickets (waves that share a SIMD take fewer)
print("blocks per wave: min %d  max %d  mean %.2f  (%d waves)" % (v[20], v[21], v[22] / max(v[23], 1), v[23]))
print("kernel ms", {k: round(t / c_, 3) for k, (c_, t) in prof.items()})
shard_table(rds, "k_lz4_encode")

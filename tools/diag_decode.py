"""Decoder time split from the diagnostic build's ablations (wrong output,
timing only): 0 full, 8 no inverse transpose/stores, 64 no sequence
execution, 72 neither, 1024 no literal copies, 2048 no match copies; then
k_lz4_decode's s_memtime phase split of a full decode (cycles per block,
summed over waves; the clock reads themselves add a little to every phase).
Last line: the blocks each wave took (equal under the static schedule,
variant 16777216; spread under tickets).
Then the per-shard finish table of that decode (variant 67108864 = no
stealing between ticket shards).  BSHUF_DIAG_SKEW=s: noise in the blocks =
s (mod 8), zeros elsewhere.
Usage: python tools/diag_decode.py [GiB] [gen] [variant]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("BSHUF_LIB", os.path.join(ROOT, "bitshuffle_amd", "libbitshuffle_mi355x_diag.so"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bitshuffle_amd as B  # noqa: E402
from bitshuffle_amd import api  # noqa: E402
import bench  # noqa: E402

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
if len(sys.argv) > 3:
    assert B.lib.bshuf_set_variant(int(sys.argv[3])) == 0
n = int(gib * (1 << 30)) // (2 if gen == 1 else 4)
x = torch.empty(n, dtype=torch.int16 if gen == 1 else torch.float32, device="cuda")
B.synth_fill_dev(x, gen)
if os.environ.get("BSHUF_DIAG_SKEW"):
    skew(x, int(os.environ["BSHUF_DIAG_SKEW"]))
c = api.compress_lz4_dev(x)
abl = B.lib.bshuf_diag_set_ablation
abl.argtypes = [ctypes.c_int]
for v in (0, 8, 64, 72, 1024, 2048, 0):
    abl(v)
    y, r = api.decompress_lz4_dev(c, x.shape, x.dtype, sync=False)
    torch.cuda.synchronize()
    B.lib.bshuf_prof_enable(1)
    bench.prof_collect(B.lib)
    for _ in range(3):
        y, r = api.decompress_lz4_dev(c, x.shape, x.dtype, sync=False)
    torch.cuda.synchronize()
    k = bench.prof_collect(B.lib)
    B.lib.bshuf_prof_enable(0)
    print("ablation %2d" % v, {name: round(ms / cnt, 3) for name, (cnt, ms) in k.items() if ms / cnt > 0.02})
abl(0)

rd = B.lib.bshuf_diag_read_dec
rd.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
buf = (ctypes.c_ulonglong * 20)()
rd(buf)
rds = B.lib.bshuf_diag_read_shards_dec
rds.argtypes = [ctypes.c_void_p]
rds((ctypes.c_ulonglong * 640)())
y, r = api.decompress_lz4_dev(c, x.shape, x.dtype, sync=False)
torch.cuda.synchronize()
rd(buf)
blocks = max(1, buf[8 + 3])
names = ["fields", "literals", "matches", "untranspose+store", "next record", "other"]
tot = sum(buf[i] for i in range(6))
for i, nm in enumerate(names):
    print("%-18s %8d cyc/block %5.1f%%" % (nm, buf[i] // blocks, 100.0 * buf[i] / max(1, tot)))
print("blocks %d  sequences/block %.1f  batches/block %.1f  coop matches/block %.1f" % (
    blocks, buf[8] / blocks, buf[9] / blocks, buf[10] / blocks))
print("blocks per wave: min %d  max %d  mean %.2f  (%d waves)" % (
    buf[16], buf[17], buf[18] / max(buf[19], 1), buf[19]))
shard_table(rds, "k_lz4_decode")

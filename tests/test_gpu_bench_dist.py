"""bench.py's multi-GPU branch on the hardware.

The driver's 8-GPU scaling run goes through bench.py's torch.distributed
path: every rank joins an RCCL ("nccl") process group, and the barrier around
the timed region plus the MAX / SUM all-reduces run on DEVICE tensors.  With
one GPU here, that path is exercised at world size 1: bench.py is started by
torch.distributed.run with --nproc-per-node=1 and --force-dist, which
initialises the RCCL group and runs every collective even for one rank.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_bench_rccl_path_world1():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", "--master-port=%d" % _free_port(),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--gib", "0.25", "--full", "--no-cpu-baseline", "--force-dist"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["dist"] == {"backend": "nccl", "world_size": 1,
                            "collectives": "barrier + all_reduce MAX/SUM on device tensors"}
    assert line["n_gpus"] == 1 and line["value"] > 0
    assert line["parity"]["round_trip_exact"] is True


@pytest.mark.timeout(120)
def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path, oracle):
    """A plain run (no --full) times --steps steps, carries none of the --full
    figures, and --dump-outputs writes the last step's stream and decoded array:
    32 MiB of int16 G1 (both dumped arrays exceed DUMP_ELEMS, so both are
    sampled), checked element for element against the CPU
    oracle at the dump's fixed sample positions."""
    import numpy as np

    import bench
    gib = 1.0 / 32
    d = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--gib", str(gib), "--dump-outputs", d]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "GiB/s"
    assert line["parity"] is None and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["kernels_avg_ms"] == {}

    n = int(gib * (1 << 30)) // 2
    a = oracle.gen_g1(n, 0, 12345)
    want = oracle.compress_lz4(a)
    assert sorted(os.listdir(d)) == ["compressed.npy", "compressed_len.npy", "decoded.npy"]
    clen = np.load(os.path.join(d, "compressed_len.npy"))
    assert clen.dtype == np.float64 and clen.tolist() == [float(want.size)]
    assert line["config"]["compressed_bytes_rank0"] == want.size
    k = bench.DUMP_ELEMS
    assert n > k and want.size > k  # both arrays are sampled
    dec = np.load(os.path.join(d, "decoded.npy"))
    assert dec.dtype == np.float32 and dec.shape == (k,)
    assert np.array_equal(dec, a[bench.sample_indices(n, k, bench.DUMP_SEED)].astype(np.float32))
    comp = np.load(os.path.join(d, "compressed.npy"))
    assert comp.dtype == np.float32 and comp.shape == (k,)
    idx = bench.sample_indices(want.size, k, bench.DUMP_SEED)
    assert idx[0] == 0 and idx[-1] == want.size - 1
    assert np.array_equal(comp, want[idx].astype(np.float32))

"""Dynamic block scheduling of the persistent LZ4 kernels (ticket counters in
the call's workspace, csrc/launch.h): which wave takes a block must not show
in any output.  Every case compares the compressed bytes with the oracle's and
the round trip with the input, at block counts around the resident grids of
both kernels (1,536 encoder and 4,608 decoder waves on MI355X), through every
launcher that owns a set of counters, with dirty and reused workspaces, and
with the static schedule (bshuf_set_variant bit 1 << 24) for comparison.

int16 with block_size = 64 elements (128-byte blocks) keeps tens of thousands
of blocks within megabytes.  By default the decoder draws tickets only for
blocks of 2 KiB and more (the encoder always), so every case that decodes runs
twice: as shipped, and with bit 1 << 25, which makes every launch draw tickets.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 64            # elements per block
PARTIAL = 40          # elements of the partial last block (a multiple of 8)
TAIL = 5              # raw tail elements
STATIC = 1 << 24      # bshuf_set_variant bit: static block assignment
TICKETS = 1 << 25     # bshuf_set_variant bit: tickets in both kernels at every block size
NO_PIPE = 1 << 20     # bshuf_set_variant bit: encode without segments
COUNTS = [1, 2, 7, 8, 9, 1535, 1536, 1537, 3073, 4607, 4608, 4609, 13827]
PIPE_BLOCKS = 65536 + 5
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def bs():
    import bitshuffle_amd
    assert bitshuffle_amd.using_HIP(), "no HIP device: the GPU suite must run on MI355X"
    return bitshuffle_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=[0, TICKETS], ids=["default", "tickets"])
def sched(request, bs):
    """Runs the test as shipped and with tickets forced on; yields the variant bit."""
    assert bs.lib.bshuf_set_variant(request.param) == 0
    yield request.param
    assert bs.lib.bshuf_set_variant(0) == 0


def n_elems(nblocks, block=BLOCK):
    """Elements of a stream of `nblocks` blocks: full ones, a partial one, a raw tail."""
    return (nblocks - 1) * block + PARTIAL + TAIL


@pytest.fixture(scope="module")
def data(oracle):
    """G1-like int16 from the oracle's generator with all-zero and random
    128-byte blocks mixed in (about one block in 16 each, and runs of them),
    so that block times differ.  Read-only; the cases take prefixes of it."""
    n = n_elems(PIPE_BLOCKS)
    a = oracle.gen_g1(n).copy()
    rng = np.random.default_rng(2024)
    nb = n // BLOCK
    blocks = a[: nb * BLOCK].reshape(nb, BLOCK)
    kind = rng.integers(0, 16, nb)
    kind[100:140] = 0      # a run of empty blocks
    kind[1500:1560] = 1    # a run of incompressible ones across the encoder's grid size
    blocks[kind == 0] = 0
    noise = rng.integers(-32768, 32768, (int((kind == 1).sum()), BLOCK)).astype(np.int16)
    blocks[kind == 1] = noise
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def streams(oracle, data):
    """nblocks -> (input prefix, the oracle's compressed stream), computed once."""
    cache = {}

    def get(nblocks):
        if nblocks not in cache:
            a = data[: n_elems(nblocks)]
            cache[nblocks] = (a, oracle.compress_lz4(a, BLOCK))
        return cache[nblocks]
    return get


def round_trip(bs, torch, a, want, block=BLOCK):
    x = torch.from_numpy(a.copy()).cuda()
    c = bs.compress_lz4_dev(x, block)
    assert c.cpu().numpy().tobytes() == want.tobytes(), "compressed bytes differ from the oracle"
    y = bs.decompress_lz4_dev(c, x.shape, x.dtype, block)
    assert torch.equal(x, y), "round trip differs from the input"


# 1. block counts around the resident grids (7, 8, 9: the shard mapping)
@pytest.mark.parametrize("nblocks", COUNTS)
def test_counts_around_the_grids(bs, torch, streams, sched, nblocks):
    a, want = streams(nblocks)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(a.size, 2, BLOCK)) == nblocks
    round_trip(bs, torch, a, want)


# 2. pipelined encode: eight launches, each with its own counters; and unsegmented
@pytest.mark.parametrize("variant", [0, NO_PIPE])
def test_pipelined_and_unsegmented_encode(bs, torch, streams, sched, variant):
    a, want = streams(PIPE_BLOCKS)
    assert bs.lib.bshuf_set_variant(variant | sched) == 0
    round_trip(bs, torch, a, want)


# 3. caller workspaces full of 0xFF, reused back to back without a host sync
@pytest.mark.parametrize("nblocks", [4609, PIPE_BLOCKS])
def test_dirty_reused_workspace(bs, torch, oracle, streams, sched, nblocks):
    a, want = streams(nblocks)
    b = a.copy()
    b[: b.size // 2] = a[b.size - b.size // 2:]  # a second input of the same size
    want_b = oracle.compress_lz4(b, BLOCK)
    x = [torch.from_numpy(v.copy()).cuda() for v in (a, b)]
    cap = bs.compress_lz4_bound(a.size, 2, BLOCK)
    ws = bs.api.compress_lz4_workspace(a.size, 2, BLOCK)
    ws.fill_(0xFF)
    bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in x]
    res = [bs.compress_lz4_dev(xi, BLOCK, out=o, workspace=ws, sync=False)[1] for xi, o in zip(x, bufs)]
    ws2 = bs.api.decompress_lz4_workspace(cap, a.size, 2, BLOCK)
    ws2.fill_(0xFF)
    dec = [bs.decompress_lz4_dev(o, xi.shape, xi.dtype, BLOCK, workspace=ws2, sync=False, length=r)
           for xi, o, r in zip(x, bufs, res)]
    torch.cuda.synchronize()
    for xi, o, r, (y, dr), w in zip(x, bufs, res, dec, (want, want_b)):
        assert int(r.item()) == w.size == int(dr.item())
        assert o[: w.size].cpu().numpy().tobytes() == w.tobytes()
        assert torch.equal(xi, y)


# 4. device-held length, capacity = the bound: blocks past the real end are drawn and dropped
@pytest.mark.parametrize("nblocks", [9, 4609, 13827])
def test_device_held_length(bs, torch, streams, sched, nblocks):
    a, want = streams(nblocks)
    x = torch.from_numpy(a.copy()).cuda()
    buf = torch.zeros(bs.compress_lz4_bound(a.size, 2, BLOCK), dtype=torch.uint8, device="cuda")
    _, res = bs.compress_lz4_dev(x, BLOCK, out=buf, sync=False)
    y, r = bs.decompress_lz4_dev(buf, x.shape, x.dtype, BLOCK, sync=False, length=res)
    assert int(res.item()) == want.size == int(r.item())
    assert buf[: want.size].cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(x, y)


# 5. batch API with device-held lengths
@pytest.mark.parametrize("chunks", [(1, 1537, 4609), (30000, 5, 30000, 5535)])
def test_batch(bs, torch, oracle, data, sched, chunks):
    arrs, pos = [], 0
    for nb in chunks:
        arrs.append(data[pos: pos + n_elems(nb)])
        pos += nb * BLOCK
    xs = [torch.from_numpy(v.copy()).cuda() for v in arrs]
    outs, res = bs.compress_lz4_batch_dev(xs, BLOCK, sync=False)
    dec, dres = bs.decompress_lz4_batch_dev(outs, [v.shape for v in arrs], torch.int16, BLOCK,
                                            sync=False, lengths=res)
    want = [oracle.compress_lz4(v, BLOCK) for v in arrs]
    assert res.cpu().tolist() == [w.size for w in want] == dres.cpu().tolist()
    for v, o, w, d in zip(arrs, outs, want, dec):
        assert o[: w.size].cpu().numpy().tobytes() == w.tobytes()
        assert d.cpu().numpy().tobytes() == v.tobytes()


# 6. the static switch: same bytes, and the bit stays outside the variant values
@pytest.mark.parametrize("nblocks,extra", [(9, 0), (1537, 0), (4609, 0), (PIPE_BLOCKS, 0),
                                           (PIPE_BLOCKS, NO_PIPE)])
def test_static_switch_same_bytes(bs, torch, streams, nblocks, extra):
    a, want = streams(nblocks)
    try:
        assert bs.lib.bshuf_set_variant(STATIC | extra) == 0
        round_trip(bs, torch, a, want)
    finally:
        bs.lib.bshuf_set_variant(0)


def test_static_switch_is_a_side_bit(bs):
    try:
        assert bs.lib.bshuf_set_variant(STATIC) == 0
        assert bs.lib.bshuf_set_variant(STATIC | 3) == -71
        assert bs.lib.bshuf_set_variant(TICKETS) == 0
        assert bs.lib.bshuf_set_variant(TICKETS | 3) == -71
    finally:
        assert bs.lib.bshuf_set_variant(0) == 0


# 7. error path: one corrupted record near the end of 4,609 blocks
def test_corrupt_record_gives_the_oracles_code(bs, torch, oracle, streams, sched):
    a, want = streams(4609)
    bad = want.copy()
    pos, k = 0, 0
    while True:  # header walk to the first record of >= 16 bytes from block 4590 on
        clen = int.from_bytes(bad[pos:pos + 4].tobytes(), "big")
        if k >= 4590 and clen >= 16:
            break
        pos, k = pos + 4 + clen, k + 1
    assert k < 4608
    bad[pos + 4: pos + 12] = 0xFF  # token 0xFF + 255-runs: literal length past the block
    with pytest.raises(RuntimeError) as orc:
        oracle.decompress_lz4(bad, a.shape, np.int16, BLOCK)
    with pytest.raises(RuntimeError) as got:
        bs.decompress_lz4_dev(torch.from_numpy(bad).cuda(), a.shape, torch.int16, BLOCK)
    assert got.value.args[1] == orc.value.args[1] < 0


# 8. default blocks and other element sizes (E = 3: the staged EK == 0 path)
@pytest.mark.parametrize("E,nblocks", [(2, 4609), (3, 1537), (4, 1537)])
def test_default_blocks_and_element_sizes(bs, torch, oracle, sched, E, nblocks):
    block = int(bs.default_block_size(E))
    n = n_elems(nblocks, block)
    raw = oracle.gen_g1((n * E + 1) // 2, 0, 777 + E).view(np.uint8)[: n * E].copy()
    rng = np.random.default_rng(E)
    rows = raw[: (nblocks - 1) * block * E].reshape(nblocks - 1, block * E)
    rows[rng.integers(0, nblocks - 1, 24)] = 0
    noisy = rng.integers(0, nblocks - 1, 24)
    rows[noisy] = rng.integers(0, 256, (24, block * E), dtype=np.uint8)
    a = raw.view(DTYPES[E]) if E in DTYPES else raw.view(np.dtype("V%d" % E))
    want = oracle.compress_lz4(a, 0)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(n, E, 0)) == nblocks
    x = torch.from_numpy(raw).cuda()
    c = bs.compress_lz4_dev(x, elem_size=E)
    assert c.cpu().numpy().tobytes() == want.tobytes()
    y = bs.decompress_lz4_dev(c, (n,), torch.uint8, elem_size=E)
    assert torch.equal(x, y)

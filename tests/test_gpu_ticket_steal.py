"""Ticket stealing between the shards of the persistent LZ4 kernels' block
counters (csrc/bshuf_dev.h, struct Tickets): a wave whose own shard has run out
draws from the shard with the most blocks left.  Which wave takes a block must
not show in any output, so every case compares the compressed bytes with the
oracle's and the round trip with the input.

The data is skewed by shard: blocks whose index is s (mod 8) hold
incompressible noise, all others zeros, so seven shards run out early and
their waves must steal from the slow one.  int16 with block_size = 64 elements
(128-byte blocks) keeps tens of thousands of blocks within megabytes.  By
default the decoder draws tickets only for blocks of 2 KiB and more and the
encoder steals only on blocks of 1 KiB and more, so every case runs as shipped
and with bit 1 << 25 (tickets, and stealing, in every launch that has them;
the decoder draws tickets but never steals).  Bit 1 << 26 switches stealing
off.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 64            # elements per block
PARTIAL = 40          # elements of the partial last block (a multiple of 8)
TAIL = 5              # raw tail elements
TICKETS = 1 << 25     # bshuf_set_variant bit: tickets in both kernels at every block size
NO_STEAL = 1 << 26    # bshuf_set_variant bit: a wave leaves when its own shard runs out
NO_PIPE = 1 << 20     # bshuf_set_variant bit: encode without segments
PIPE_BLOCKS = 65536 + 5
SKEWS = [0, 3, 7]
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
def skewed():
    """s -> int16 array of PIPE_BLOCKS blocks: noise in blocks = s (mod 8), zeros
    elsewhere (the partial block and the tail: noise).  Read-only; cases take prefixes."""
    cache = {}

    def get(s):
        if s not in cache:
            n = n_elems(PIPE_BLOCKS)
            rng = np.random.default_rng(4242 + s)
            a = np.zeros(n, dtype=np.int16)
            nb = n // BLOCK
            rows = a[: nb * BLOCK].reshape(nb, BLOCK)
            slow = np.arange(nb) % 8 == s
            rows[slow] = rng.integers(-32768, 32768, (int(slow.sum()), BLOCK)).astype(np.int16)
            a[nb * BLOCK:] = rng.integers(-32768, 32768, n - nb * BLOCK).astype(np.int16)
            a.setflags(write=False)
            cache[s] = a
        return cache[s]
    return get


@pytest.fixture(scope="module")
def streams(oracle, skewed):
    """(s, nblocks) -> (input prefix, the oracle's compressed stream), computed once."""
    cache = {}

    def get(s, nblocks):
        if (s, nblocks) not in cache:
            a = skewed(s)[: n_elems(nblocks)]
            cache[(s, nblocks)] = (a, oracle.compress_lz4(a, BLOCK))
        return cache[(s, nblocks)]
    return get


def round_trip(bs, torch, a, want, block=BLOCK):
    x = torch.from_numpy(a.copy()).cuda()
    c = bs.compress_lz4_dev(x, block)
    assert c.cpu().numpy().tobytes() == want.tobytes(), "compressed bytes differ from the oracle"
    y = bs.decompress_lz4_dev(c, x.shape, x.dtype, block)
    assert torch.equal(x, y), "round trip differs from the input"


# 1. skewed shards: the seven fast shards run out and steal from the slow one
@pytest.mark.parametrize("s", SKEWS)
@pytest.mark.parametrize("nblocks", [1537, 4609, 13827])
def test_skewed_shards(bs, torch, streams, sched, nblocks, s):
    a, want = streams(s, nblocks)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(a.size, 2, BLOCK)) == nblocks
    round_trip(bs, torch, a, want)


# ... through the pipelined encode (eight launches, eight counter sets) and unsegmented
@pytest.mark.parametrize("s", SKEWS)
@pytest.mark.parametrize("variant", [0, NO_PIPE])
def test_skewed_pipelined_and_unsegmented(bs, torch, streams, sched, variant, s):
    a, want = streams(s, PIPE_BLOCKS)
    assert bs.lib.bshuf_set_variant(variant | sched) == 0
    round_trip(bs, torch, a, want)


# 2. shards that own nothing: G+1 .. G+7 blocks for both grids, and 2 .. 9
@pytest.mark.parametrize("nblocks", list(range(2, 10)) + list(range(1537, 1544)) + list(range(4609, 4616)))
def test_shards_that_own_nothing(bs, torch, streams, sched, nblocks):
    a, want = streams(3, nblocks)
    round_trip(bs, torch, a, want)


# 3. caller workspaces full of 0xFF, reused back to back without a host sync:
#    over-drawn counters must not leak into the next call
@pytest.mark.parametrize("nblocks", [4609, PIPE_BLOCKS])
def test_dirty_reused_workspace(bs, torch, oracle, streams, sched, nblocks):
    a, want = streams(3, nblocks)
    b, want_b = streams(7, nblocks)  # a second input of the same size
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
@pytest.mark.parametrize("s", SKEWS)
@pytest.mark.parametrize("nblocks", [9, 4609, 13827])
def test_device_held_length(bs, torch, streams, sched, nblocks, s):
    a, want = streams(s, nblocks)
    x = torch.from_numpy(a.copy()).cuda()
    buf = torch.zeros(bs.compress_lz4_bound(a.size, 2, BLOCK), dtype=torch.uint8, device="cuda")
    _, res = bs.compress_lz4_dev(x, BLOCK, out=buf, sync=False)
    y, r = bs.decompress_lz4_dev(buf, x.shape, x.dtype, BLOCK, sync=False, length=res)
    assert int(res.item()) == want.size == int(r.item())
    assert buf[: want.size].cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(x, y)


# 5. batch API with device-held lengths on skewed chunks
@pytest.mark.parametrize("s", SKEWS)
def test_batch(bs, torch, oracle, skewed, sched, s):
    data = skewed(s)
    arrs, pos = [], 0
    for nb in (1, 1537, 4609):
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


# 6. error path: one corrupted record in the last 20 blocks of 4,609
def test_corrupt_record_gives_the_oracles_code(bs, torch, oracle, streams, sched):
    a, want = streams(3, 4609)
    bad = want.copy()
    pos, k = 0, 0
    while True:  # header walk to the first record of >= 16 bytes from block 4590 on
        clen = int.from_bytes(bad[pos:pos + 4].tobytes(), "big")
        if k >= 4590 and clen >= 16:
            break
        pos, k = pos + 4 + clen, k + 1
    assert 4589 <= k < 4608
    bad[pos + 4: pos + 12] = 0xFF  # token 0xFF + 255-runs: literal length past the block
    with pytest.raises(RuntimeError) as orc:
        oracle.decompress_lz4(bad, a.shape, np.int16, BLOCK)
    with pytest.raises(RuntimeError) as got:
        bs.decompress_lz4_dev(torch.from_numpy(bad).cuda(), a.shape, torch.int16, BLOCK)
    assert got.value.args[1] == orc.value.args[1] < 0


# 7. the no-stealing switch: same bytes, and the bit stays outside the variant values
@pytest.mark.parametrize("nblocks,extra", [(9, 0), (1537, 0), (4609, 0), (4609, TICKETS),
                                           (PIPE_BLOCKS, 0), (PIPE_BLOCKS, NO_PIPE)])
def test_no_stealing_same_bytes(bs, torch, streams, nblocks, extra):
    a, want = streams(3, nblocks)
    try:
        assert bs.lib.bshuf_set_variant(NO_STEAL | extra) == 0
        round_trip(bs, torch, a, want)
    finally:
        bs.lib.bshuf_set_variant(0)


def test_no_stealing_is_a_side_bit(bs):
    try:
        assert bs.lib.bshuf_set_variant(NO_STEAL) == 0
        assert bs.lib.bshuf_set_variant(NO_STEAL | 3) == -71
    finally:
        assert bs.lib.bshuf_set_variant(0) == 0


# 8. default 8 KiB blocks, skewed, and other element sizes (E = 3: the staged EK == 0 path)
@pytest.mark.parametrize("s", SKEWS)
@pytest.mark.parametrize("E,nblocks", [(2, 4609), (3, 1537), (4, 1537)])
def test_default_blocks_skewed(bs, torch, oracle, sched, E, nblocks, s):
    block = int(bs.default_block_size(E))
    n = n_elems(nblocks, block)
    rng = np.random.default_rng(100 * E + s)
    raw = np.zeros(n * E, dtype=np.uint8)
    rows = raw[: (nblocks - 1) * block * E].reshape(nblocks - 1, block * E)
    slow = np.arange(nblocks - 1) % 8 == s
    rows[slow] = rng.integers(0, 256, (int(slow.sum()), block * E), dtype=np.uint8)
    raw[(nblocks - 1) * block * E:] = rng.integers(0, 256, (PARTIAL + TAIL) * E, dtype=np.uint8)
    a = raw.view(DTYPES[E]) if E in DTYPES else raw.view(np.dtype("V%d" % E))
    want = oracle.compress_lz4(a, 0)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(n, E, 0)) == nblocks
    x = torch.from_numpy(raw).cuda()
    c = bs.compress_lz4_dev(x, elem_size=E)
    assert c.cpu().numpy().tobytes() == want.tobytes()
    y = bs.decompress_lz4_dev(c, (n,), torch.uint8, elem_size=E)
    assert torch.equal(x, y)

"""GPU tests of the fast encode mode (mode="fast", bshuf_compress_lz4_fast*):
the stream equals the numpy model of "fast parse v1" (tests/fast_model.py)
byte for byte, the existing decoder takes it back to the input, and the single,
batch, host and segmented entries agree.  Byte work: every comparison is exact."""
import ctypes

import numpy as np
import pytest

from tests import fast_cases, fast_model

pytestmark = pytest.mark.gpu


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


def _case_ids():
    ids = []
    for E, n in fast_cases.SHAPES:
        ids += ["E%d_n%d_%s" % (E, n, k) for k in fast_cases.KINDS]
    return ids + ["many_sequences", "bs8", "bs64", "bs680", "bs680_zeros", "bs16384", "bs32768",
                  "bs32768_zeros", "E4_bs16384"]


@pytest.fixture(scope="module")
def cases(oracle):
    return {c[0]: c for c in fast_cases.cases(oracle)}


def _fast_dev(bs, torch, raw, E, bsz, **kw):
    x = torch.from_numpy(raw).cuda()
    return bs.compress_lz4_dev(x, bsz, elem_size=E, mode="fast", **kw)


@pytest.mark.parametrize("name", _case_ids())
def test_fast_stream_equals_model_and_decodes(bs, oracle, torch, cases, name):
    _, raw, E, bsz = cases[name]
    arr = fast_cases.view_e(raw, E)
    want = fast_model.compress_lz4(oracle, arr, bsz)
    x = torch.from_numpy(raw).cuda()
    res = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    got = bs.compress_lz4_dev(x, bsz, elem_size=E, mode="fast", result=res)
    assert int(res.item()) == got.numel() == want.size
    assert got.cpu().numpy().tobytes() == want.tobytes()
    back = bs.decompress_lz4_dev(got, (arr.size,), None, bsz, elem_size=E)
    assert back.cpu().numpy().tobytes() == raw.tobytes()


def test_default_mode_is_untouched(bs, oracle, torch, cases):
    _, raw, E, bsz = cases["E2_n12365_gen"]
    x = torch.from_numpy(raw).cuda()
    want = oracle.compress_lz4(fast_cases.view_e(raw, E)).tobytes()
    assert bs.compress_lz4_dev(x, elem_size=E).cpu().numpy().tobytes() == want
    assert bs.compress_lz4_dev(x, elem_size=E, mode="exact").cpu().numpy().tobytes() == want
    assert want != fast_model.compress_lz4(oracle, fast_cases.view_e(raw, E)).tobytes()


def test_blocks_above_the_limit_take_the_exact_parse(bs, oracle, torch):
    _, raw, E, bsz = fast_cases.big_block_case(oracle)
    assert bsz * E > fast_model.FAST_MAX_BLOCK_BYTES
    arr = fast_cases.view_e(raw, E)
    want = oracle.compress_lz4(arr, bsz)
    got = _fast_dev(bs, torch, raw, E, bsz)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert fast_model.compress_lz4(oracle, arr, bsz).tobytes() == want.tobytes()
    outs = bs.compress_lz4_batch_dev([torch.from_numpy(raw).cuda()] * 2, bsz, elem_size=E, mode="fast")
    assert [o.cpu().numpy().tobytes() for o in outs] == [want.tobytes()] * 2


def test_batch_equals_single_streams(bs, oracle, torch):
    """Three streams of different lengths, one shorter than a block; caller
    workspace and offsets; each equals its single-stream result."""
    g = fast_cases.gen_bytes(oracle, 2 * (3 * 4096 + 77), 1)
    raws = [g, g[:2 * 520].copy(), g[2 * 100:2 * (100 + 4096 + 8)].copy()]
    xs = [torch.from_numpy(r).view(torch.int16).cuda() for r in raws]
    singles = [bs.compress_lz4_dev(x, mode="fast").cpu().numpy().tobytes() for x in xs]
    for r, s in zip(raws, singles):
        assert s == fast_model.compress_lz4(oracle, r.view(np.int16)).tobytes()
    sizes = (ctypes.c_size_t * 3)(*[x.numel() for x in xs])
    wsb = int(bs.lib.bshuf_compress_lz4_batch_dev_workspace(ctypes.cast(sizes, ctypes.c_void_p), 3, 2, 0))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    nblk = sum(int(bs.lib.bshuf_lz4_dev_nblocks(x.numel(), 2, 0)) for x in xs)
    offs = torch.zeros(nblk, dtype=torch.int64, device="cuda")
    outs = bs.compress_lz4_batch_dev(xs, mode="fast", workspace=ws, offsets=offs)
    assert [o.cpu().numpy().tobytes() for o in outs] == singles
    assert offs.cpu().tolist()[:4] == [0] + list(np.cumsum(
        [4 + p.size for _, p in fast_model.block_records(np.frombuffer(singles[0], np.uint8), oracle,
                                                        raws[0].view(np.int16))][:3]))
    outs2, results = bs.compress_lz4_batch_dev(xs, mode="fast", sync=False)
    assert results.cpu().tolist() == [len(s) for s in singles]


def test_segmented_launches(bs, oracle, torch):
    """More than 65,536 blocks (16-byte blocks): the pipelined, segmented launch
    structure, single stream and batch."""
    _, raw, E, bsz = fast_cases.segmented_case(oracle)
    arr = fast_cases.view_e(raw, E)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(arr.size, E, bsz)) > 65536
    want = fast_model.compress_lz4(oracle, arr, bsz, cache={}).tobytes()
    x = torch.from_numpy(raw).view(torch.int16).cuda()
    got = bs.compress_lz4_dev(x, bsz, mode="fast")
    assert got.cpu().numpy().tobytes() == want
    back = bs.decompress_lz4_dev(got, (arr.size,), torch.int16, bsz)
    assert back.cpu().numpy().tobytes() == raw.tobytes()
    half = x[:40000 * 8 + 16]
    outs = bs.compress_lz4_batch_dev([x, half], bsz, mode="fast")
    assert outs[0].cpu().numpy().tobytes() == want
    assert outs[1].cpu().numpy().tobytes() == bs.compress_lz4_dev(half, bsz, mode="fast").cpu().numpy().tobytes()


def test_unsynchronised_chain_into_decode(bs, oracle, torch, cases):
    """sync=False: the result word stays on the device and feeds the decoder."""
    _, raw, E, bsz = cases["E2_n12365_gen"]
    x = torch.from_numpy(raw).view(torch.int16).cuda()
    out, res = bs.compress_lz4_dev(x, mode="fast", sync=False)
    back, used = bs.decompress_lz4_dev(out, (x.numel(),), torch.int16, length=res, sync=False)
    want = fast_model.compress_lz4(oracle, raw.view(np.int16))
    assert int(res.item()) == int(used.item()) == want.size
    assert torch.equal(back, x)
    assert out[:want.size].cpu().numpy().tobytes() == want.tobytes()


def test_caller_workspace_and_offsets(bs, oracle, torch, cases):
    _, raw, E, bsz = cases["E4_n4104_gen"]
    x = torch.from_numpy(raw).view(torch.int32).cuda()
    ws = bs.api.compress_lz4_workspace(x.numel(), 4)
    nb = int(bs.lib.bshuf_lz4_dev_nblocks(x.numel(), 4, 0))
    offs = torch.zeros(nb, dtype=torch.int64, device="cuda")
    got = bs.compress_lz4_dev(x, mode="fast", workspace=ws, offsets=offs)
    want = fast_model.compress_lz4(oracle, raw.view(np.uint32))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    recs = fast_model.block_records(want, oracle, raw.view(np.uint32))
    assert offs.cpu().tolist() == [0] + list(np.cumsum([4 + p.size for _, p in recs])[:-1])
    # the decoder takes the offsets of a fast stream like any other
    back = bs.decompress_lz4_dev(got, (x.numel(),), torch.int32, offsets=offs)
    assert torch.equal(back, x)


def test_host_entry(bs, oracle, cases):
    for name in ("E2_n12365_gen", "E3_n5480_period3", "E1_n8_random", "E2_n5_gen"):
        _, raw, E, bsz = cases[name]
        arr = fast_cases.view_e(raw, E)
        got = bs.compress_lz4(arr, mode="fast")
        assert got.tobytes() == fast_model.compress_lz4(oracle, arr).tobytes(), name
        assert bs.decompress_lz4(got, arr.shape, arr.dtype).tobytes() == arr.tobytes(), name


def test_errors(bs, torch):
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.empty(1024, dtype=torch.uint8, device="cuda")
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert bs.lib.bshuf_compress_lz4_fast_dev(p(x), p(out), 64, 0, 0, None, 0, p(res), None, None) == -71
    assert bs.lib.bshuf_compress_lz4_fast_dev(p(x), p(out), 64, 2, 12, None, 0, p(res), None, None) == -81
    # a caller workspace that is too small
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    assert bs.lib.bshuf_compress_lz4_fast_dev(p(x), p(out), 64, 2, 0, p(ws), 256, p(res), None, None) == -71
    for fn in (bs.compress_lz4_dev, lambda t, **k: bs.compress_lz4_batch_dev([t], **k)):
        with pytest.raises(ValueError):
            fn(x, mode="quick")
    with pytest.raises(ValueError):
        bs.compress_lz4(np.zeros(64, dtype=np.int16), mode=None)

"""The fixtures and the runner the crafted-block GPU tests share (test_gpu_emit_shapes.py,
test_gpu_search_cases.py).  Test infrastructure only."""
import numpy as np
import pytest

from tests.emit_cases import view


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


@pytest.fixture
def variant(bs):
    """Sets a bshuf_set_variant value; 0 is restored behind the test."""
    def set_(v):
        assert bs.lib.bshuf_set_variant(v) == 0, v
    yield set_
    assert bs.lib.bshuf_set_variant(0) == 0


def run_case(bs, torch, oracle, variant, blocks, E, block_elems, block_arg=0, tail=b"", variants=(0,)):
    """Shuffled blocks (+ raw tail bytes) -> input -> device stream == oracle
    stream under every bshuf_set_variant value of `variants`, then decoded
    back.  -> (input array, oracle stream)."""
    sh = np.concatenate(list(blocks) + [np.frombuffer(tail, np.uint8)])
    a = oracle.bitunshuffle(view(sh, E), block_elems)
    want = oracle.compress_lz4(a, block_arg)
    raw = a.view(np.uint8).reshape(-1)
    x = torch.from_numpy(raw.copy()).cuda()
    for v in variants:
        variant(v)
        c = bs.compress_lz4_dev(x, block_arg, elem_size=E)
        assert c.cpu().numpy().tobytes() == want.tobytes(), v
    y = bs.decompress_lz4_dev(c, (raw.size // E,), torch.uint8, block_arg, elem_size=E)
    assert torch.equal(x, y)
    return a, want

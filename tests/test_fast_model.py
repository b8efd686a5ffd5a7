"""CPU tests of the fast encode mode ("fast parse v1"): the
numpy model of the rule (tests/fast_model.py) produces valid LZ4 that the
oracle's and the reference's decoders take back to the input, stays within a
tenth of the reference encoder's size on the project's inputs, and the new
C-ABI symbols exist and fail loudly without a GPU."""
import ctypes

import numpy as np
import pytest

import oracle as oracle_mod
from tests import fast_cases, fast_model


@pytest.fixture(scope="module")
def reference():
    return oracle_mod.Reference() if oracle_mod.reference_available() else None


def _all_cases(oracle):
    return fast_cases.cases(oracle) + [fast_cases.big_block_case(oracle)]


def test_model_streams_are_valid(oracle, reference):
    """Every block payload decodes (oracle, and the reference's
    LZ4_decompress_safe when built) to the bit-transposed block, the framed
    stream decodes to the input, and every record keeps the exact encoder's
    bound 4 + L + L/255 + 16."""
    for name, raw, E, bsz in _all_cases(oracle):
        arr = fast_cases.view_e(raw, E)
        stream = fast_model.compress_lz4(oracle, arr, bsz)
        assert stream.size <= oracle.compress_lz4_bound(arr.size, E, bsz), name
        back = oracle.decompress_lz4(stream, arr.shape, arr.dtype, bsz)
        assert back.tobytes() == arr.tobytes(), name
        bs = bsz or oracle.default_block_size(E)
        shuf = oracle.bitshuffle(arr, bs).view(np.uint8).reshape(-1) if arr.size else raw
        pos = 0
        for L, payload in fast_model.block_records(stream, oracle, arr, bsz):
            assert 4 + payload.size <= 4 + L + L // 255 + 16, name
            want = shuf[pos:pos + L].tobytes()
            assert oracle.lz4_decompress_block(payload, L).tobytes() == want, name
            if reference is not None:
                assert reference.lz4_decompress_block(payload, L).tobytes() == want, name
            pos += L


def test_model_size_within_a_tenth_of_the_reference(oracle):
    """Framed size of the fast parse <= 1.10 x the reference-pinned oracle's on
    the six inputs of DESIGN.md §6.6's ratio table."""
    for label, gen, E, nblocks in fast_cases.RATIO_INPUTS:
        arr = fast_cases.ratio_input(oracle, gen, E, nblocks)
        fast = fast_model.compress_lz4(oracle, arr).size
        exact = len(oracle.compress_lz4(arr))
        print("%-18s E=%-2d fast %8d exact %8d ratio %.4f" % (label, E, fast, exact, fast / exact))
        assert fast <= 1.10 * exact, (label, fast, exact)


def test_spot_values(oracle):
    # 8192 zero int16: two blocks, each one literal + one block-long match at
    # offset 1 + the last 5 literals -- the exact encoder's parse as well
    z = np.zeros(8192, dtype=np.int16)
    s = fast_model.compress_lz4(oracle, z)
    assert s.size == 94
    assert s.tobytes() == oracle.compress_lz4(z).tobytes()
    # uniform random bytes: no run of 4 at any offset, literal-only blocks
    r = np.random.default_rng(5).integers(0, 256, 3 * 8192, dtype=np.uint8)
    s = fast_model.compress_lz4(oracle, r)
    assert s.size == len(oracle.compress_lz4(r)) == 3 * (4 + 8192 + 1 + (8192 - 15) // 255 + 1)
    for L, payload in fast_model.block_records(s, oracle, r):
        assert fast_model.parse(oracle.lz4_decompress_block(payload, L), 1) == [(0, L, 0, 0)]


def test_offset_set():
    assert fast_model.offsets(8192, 2) == [1, 2, 3, 4, 8, 512, 1024]
    assert fast_model.offsets(8192, 4) == [1, 2, 3, 4, 8, 256, 512]
    assert fast_model.offsets(16, 2) == [1, 2, 3, 4, 8]      # P = 1
    assert fast_model.offsets(128, 2) == [1, 2, 3, 4, 8, 16]  # P = 8
    assert fast_model.offsets(64, 1) == [1, 2, 3, 4, 8, 16]   # P = 8
    assert fast_model.offsets(96, 3) == [1, 2, 3, 4, 8]      # P = 4, 2P = 8


def test_fast_abi_declared_and_fails_loudly():
    """The fast entries are declared, prototyped and exported; the version is
    1; a bad block size is -81 before the device is looked at, and without a
    GPU every fast entry returns -70 -- no CPU path."""
    import bitshuffle_amd as B
    from bitshuffle_amd._lib import PROTOTYPES
    from tests.test_cabi import declared_symbols
    names = ["bshuf_lz4_fast_version", "bshuf_compress_lz4_fast", "bshuf_compress_lz4_fast_dev",
             "bshuf_compress_lz4_fast_batch_dev"]
    declared = declared_symbols()
    for n in names:
        assert n in declared and n in PROTOTYPES, n
    assert B.lib.bshuf_lz4_fast_version() == 1
    assert B.FAST_PARSE_VERSION == 1 == fast_model.FAST_PARSE_VERSION
    a = np.arange(64, dtype=np.int16)
    out = np.empty(1024, dtype=np.uint8)
    pa, po = ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert B.lib.bshuf_compress_lz4_fast(pa, po, 64, 2, 12) == -81
    assert B.lib.bshuf_compress_lz4_fast_dev(None, None, 64, 2, 12, None, 0, None, None, None) == -81
    sizes = (ctypes.c_size_t * 1)(64)
    ptrs = (ctypes.c_void_p * 1)(None)
    batch = (ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p),
             ctypes.cast(sizes, ctypes.c_void_p))
    assert B.lib.bshuf_compress_lz4_fast_batch_dev(*batch, 1, 2, 12, None, 0, None, None, None) == -81
    with pytest.raises(ValueError):
        B.compress_lz4(a, mode="quick")
    if not B.using_HIP():
        assert B.lib.bshuf_compress_lz4_fast(pa, po, 64, 2, 0) == -70
        assert B.lib.bshuf_compress_lz4_fast_dev(None, None, 64, 2, 0, None, 0, None, None, None) == -70
        assert B.lib.bshuf_compress_lz4_fast_batch_dev(*batch, 1, 2, 0, None, 0, None, None, None) == -70
        with pytest.raises(RuntimeError) as ei:
            B.compress_lz4(a, mode="fast")
        assert ei.value.args[1] == -70

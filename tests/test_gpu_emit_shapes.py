"""The LZ4 encoder's emission (csrc/lz4_encode.hip, emit_sequences_flat) on the
device, byte for byte against the CPU oracle through the C-ABI.

Every case builds the SHUFFLED blocks it wants (tests/emit_cases.py: random
bytes for literal runs, byte runs for matches, lengths checked by parsing the
oracle's record) and gets the codec's input from the oracle's bitunshuffle.
A call holds 2-64 different blocks, so the batches of 64 sequences and the
deferred copy-out carry over between blocks of different shapes.  Covered:
literal runs of 0, 1, 3, 4, 5, 14-17, 63-65, 127-129, 269-271, 524, 525 and
about 3 KiB; every destination x source alignment of a run, per lane and by the
wave; runs that end at the block end; matches of 4, 18, 19, 273, 274 and
3,000 bytes; 0, 1, 63, 64, 65, 255, 256 and 257 sequences per block (257: the
inline emitter); partial blocks and 16-byte blocks; the batch API; the
unsegmented and the pipelined encode.  A block is a multiple of 8 elements, so
its byte size is always a multiple of 8: "not a multiple of 16" is covered
(24, 40, 72, 8,184 bytes), "not a multiple of 4" cannot occur.

Each case runs under the default variant and under round 5's emission
(bshuf_set_variant 3072000, the A/B partner).
"""
import numpy as np
import pytest

from tests import emit_cases as C
from tests import gpu_run
from tests.gpu_run import bs, torch, variant  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

OLD_EMIT = 3072000   # bshuf_set_variant: round 5's emission (2793472 for the odd element sizes)
NO_PIPE = 1 << 20
VARIANTS = [0, OLD_EMIT]


def run_case(bs, torch, oracle, variant, blocks, E, block_elems, block_arg=0, tail=b""):
    """Shuffled blocks (+ raw tail bytes) -> input -> device stream == oracle stream."""
    gpu_run.run_case(bs, torch, oracle, variant, blocks, E, block_elems, block_arg, tail, variants=VARIANTS)


@pytest.fixture(scope="module")
def lengths(oracle):
    """E -> (blocks, elements per block); the lengths they hold are checked."""
    out = {}
    for E in (2, 4, 3):
        blocks, be = C.length_cases(oracle, E)
        lits, mls, _ = C.coverage(oracle, blocks)
        assert set(C.LITS) <= lits and set(C.MATCHES) <= mls
        assert any(3000 <= x <= 3200 for x in lits) and any(x >= 2048 for x in mls)
        out[E] = (blocks, be)
    return out


@pytest.fixture(scope="module")
def counts(oracle):
    out = {}
    for E in (2, 4, 3):
        blocks, be, want = C.count_cases(oracle, E)
        assert C.coverage(oracle, blocks)[2] == want
        out[E] = (blocks, be)
    return out


# 1. literal-run lengths, alignments, match lengths, runs at the block end
@pytest.mark.parametrize("E", [2, 4, 3])
def test_run_and_match_lengths(bs, torch, oracle, variant, lengths, E):
    blocks, be = lengths[E]
    run_case(bs, torch, oracle, variant, blocks, E, be)
    # the same blocks in another order: another block's record is pending
    run_case(bs, torch, oracle, variant, blocks[::-1] + blocks[1::2], E, be)


# 2. sequences per block: batches of 64, the last descriptor slot, the fallback
@pytest.mark.parametrize("E", [2, 4, 3])
def test_sequence_counts(bs, torch, oracle, variant, counts, E):
    blocks, be = counts[E]
    run_case(bs, torch, oracle, variant, blocks, E, be)


# 3. a partial last block (24 .. 8,176 bytes) and raw tail elements behind it
@pytest.mark.parametrize("E,part", [(2, 8), (2, 4088), (3, 8), (3, 24), (3, 2720), (1, 40), (4, 8), (4, 2040)])
def test_partial_block_and_tail(bs, torch, oracle, variant, lengths, E, part):
    be = oracle.default_block_size(E)
    full = lengths[E][0][:3] if E in lengths else [np.random.default_rng(1).integers(0, 4, be * E, dtype=np.uint8)]
    bld = C.Builder(oracle, 100 + part)
    nb = part * E
    spec = [(3, 9), (17, 30), (5, 6)] if nb >= 200 else []
    last = bld.block(spec, nb) if nb >= 64 else bld.rng.integers(0, 2, nb, dtype=np.uint8) * 255
    run_case(bs, torch, oracle, variant, full + [last], E, be, tail=bytes(range(1, 1 + 5 * E)))


# 4. blocks of 16 and 24 bytes (8 elements), 64 of them in one call
@pytest.mark.parametrize("E", [2, 3])
def test_blocks_of_eight_elements(bs, torch, oracle, variant, E):
    rng = np.random.default_rng(E)
    kinds = [np.zeros(8 * E, np.uint8), rng.integers(0, 256, 8 * E, dtype=np.uint8),
             np.repeat(rng.integers(0, 256, 2 * E, dtype=np.uint8), 4), np.full(8 * E, 7, np.uint8)]
    blocks = [kinds[i % 4] if i % 5 else rng.integers(0, 3, 8 * E, dtype=np.uint8) for i in range(64)]
    run_case(bs, torch, oracle, variant, blocks, E, 8, block_arg=8)


# 5. the batch API: three streams of different shapes in one launch
def test_batch_of_three_shapes(bs, torch, oracle, variant, lengths, counts):
    be = oracle.default_block_size(2)
    bld = C.Builder(oracle, 31)
    part = bld.block([(15, 18), (64, 4), (270, 19)], 1200)
    shs = [np.concatenate(lengths[2][0]), np.concatenate(counts[2][0][3:7] + [part]),
           np.concatenate([lengths[2][0][2], counts[2][0][0], part[:16]])]
    arrs = [oracle.bitunshuffle(sh.view(np.int16), be) for sh in shs]
    want = [oracle.compress_lz4(a, 0) for a in arrs]
    xs = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    for v in VARIANTS:
        variant(v)
        outs = bs.compress_lz4_batch_dev(xs, 0)
        for o, w in zip(outs, want):
            assert o.cpu().numpy().tobytes() == w.tobytes(), v


# 6. 65,541 blocks of 128 bytes, unsegmented and pipelined: the record that is
# pending when a wave draws its next ticket comes from any of 41 shapes
def test_pipelined_and_unsegmented(bs, torch, oracle, variant):
    bld = C.Builder(oracle, 65)
    shapes = []
    for i in range(41):
        spec = [(1 + (i + j) % 6, 4 + (3 * i + j) % 9) for j in range(1 + i % 4)]
        shapes.append(bld.block(spec, 128, tail_lits=0 if i % 3 == 0 else None))
    idx = np.random.default_rng(3).integers(0, 41, 65541)
    sh = np.stack(shapes)[idx].reshape(-1)
    a = oracle.bitunshuffle(sh.view(np.int16), 64)
    want = oracle.compress_lz4(a, 64)
    x = torch.from_numpy(a).cuda()
    for v in (0, NO_PIPE, OLD_EMIT):
        variant(v)
        c = bs.compress_lz4_dev(x, 64)
        assert c.cpu().numpy().tobytes() == want.tobytes(), v

"""The addressing of the LZ4 encoder's wave-parallel emission, settled on the
CPU: tests/emit_model.py restates emit_sequences_flat access by access (prefix
sum, closed-form length runs, masked head / tail dwords, the per-lane interior
loop and the wave's step walk over the long runs), and must rebuild the
oracle's record byte for byte from the oracle's own parse, for the shapes the
GPU test (test_gpu_emit_shapes.py) runs.  It also checks the bounds the kernel
relies on: no interior dword written twice, every unmasked read inside the
LDS behind the block.
"""
import numpy as np
import pytest

from tests import emit_cases as C
from tests.emit_model import emit, ext_bytes, parse_record


def check_blocks(oracle, blocks, stats=None):
    for i, b in enumerate(blocks):
        rec = oracle.lz4_compress_block(b)
        seqs, la = parse_record(rec, b.size)
        got = emit(b, seqs, la, stats)
        assert got.tobytes() == rec.tobytes(), (i, len(seqs))


@pytest.mark.parametrize("E", [2, 4, 3])
def test_length_cases_hold_their_lengths_and_rebuild(oracle, E):
    blocks, _ = C.length_cases(oracle, E)
    lits, mls, _ = C.coverage(oracle, blocks)
    assert set(C.LITS) <= lits, sorted(set(C.LITS) - lits)
    assert any(3000 <= x <= 3200 for x in lits), sorted(lits)[-3:]
    assert set(C.MATCHES) <= mls, sorted(set(C.MATCHES) - mls)
    assert any(x >= 2048 for x in mls)
    stats = {}
    check_blocks(oracle, blocks, stats)
    assert stats["steps"] >= 4          # the long run: several wave steps
    assert 0 < stats["read_hi"] <= 1072  # the steps' over-read, inside the 2 KiB behind the block


@pytest.mark.parametrize("E", [2, 3])
def test_sequence_counts(oracle, E):
    blocks, _, want = C.count_cases(oracle, E)
    _, _, counts = C.coverage(oracle, blocks)
    assert counts == want
    check_blocks(oracle, blocks)


def test_every_destination_and_source_alignment(oracle):
    """lp & 3 against lsrc & 3, for per-lane runs and for wave runs."""
    blocks, _ = C.length_cases(oracle, 2)
    seen = {False: set(), True: set()}
    for b in blocks:
        seqs, la = parse_record(oracle.lz4_compress_block(b), b.size)
        op = 4
        for ip, off, lit, ml in seqs:
            lp = op + 1 + ext_bytes(lit)
            if lit > 16:
                seen[lit > 32].add((lp & 3, (ip - lit) & 3))
            op = lp + lit + 2 + ext_bytes(ml - 4)
    for wave in (False, True):
        assert len(seen[wave]) == 16, (wave, sorted(seen[wave]))


@pytest.mark.parametrize("n", [16, 24, 40, 72, 8176, 8184])
def test_small_and_odd_blocks(oracle, n):
    rng = np.random.default_rng(n)
    blocks = [np.zeros(n, np.uint8), rng.integers(0, 256, n, dtype=np.uint8),
              rng.integers(0, 2, n, dtype=np.uint8), np.repeat(rng.integers(0, 256, (n + 7) // 8, dtype=np.uint8), 8)[:n]]
    check_blocks(oracle, blocks)


def test_g1_blocks(oracle):
    a = oracle.gen_g1(4096 * 6)
    sh = oracle.bitshuffle(a).view(np.uint8).reshape(6, 8192)
    stats = {}
    check_blocks(oracle, list(sh), stats)
    assert stats["steps"] >= 4

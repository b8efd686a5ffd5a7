"""The LZ4 encoder's SEARCH (csrc/lz4_encode.hip: the probe windows, the undo
of a matching window's later inserts, the catch-up, the count windows, the
re-test, the distance rule) on the device, byte for byte against the CPU
oracle.

Every case runs the crafted shuffled blocks of tests/search_cases.py, whose
events tests/test_search_cases.py asserts on the CPU with the instrumented
serial parse (tests/parse_census.py); the codec's input comes from the
oracle's bitunshuffle.  What each family reaches in the kernel:

A  catch-up lengths.  back >= 64: search_entry returns back = -1, so the
   continuation loop behind it (`if (back < 0)`, 64 bytes per step), its twin
   in catch_and_count (`if (back == kWave)`; variants without the asm entry,
   the partial window, odd element sizes) and parse_chain's kPcEntry hand-back
   (`s_cmp_lt_i32 t4, 0` -> L_eslow).  62/63 against 64/65/66 and 127/128/129
   are the last lane of one 64-byte step and the first of the next; a
   catch-up that ends at the anchor or at position 0 ends on the `xa >=
   anchor` / `xb >= 0` term of the ballot, not on a byte.
B  probe schedule.  Lanes 0, 1, 62, 63 of windows 0, 1, 2, 4: js at both ends
   of the window's ballot (`lane > js` restores nothing at 63, everything at
   0), probe_lane's closed form across the step changes.  The block end: the
   partial window (kPcPartial, `valid`, exchange_if) with 1 and 63 valid
   lanes, a hit at its last valid lane, mpos == limit - 1, a count capped by
   mlimit and one a byte short of it, kPcLimit / kRtLimit, the re-test at
   limit - 1; blocks of 16..40 bytes around kLz4MinLength.
C  table traffic inside the hit's window: the four restore sites
   (`if (lane > js && cand <= mpos) T.put(h, cand)` in search_chain's exit,
   the compiled full window, the partial window and the general window) and
   the read-back search's group logic (variant 128), with the restored entry
   read later by a position that repeats its bytes: a wrong restore changes an
   offset of the stream.
D  count windows: kPcLong / kRtLong (a re-test whose first 256 bytes are
   equal; counts of 256 and 257 end in the second window's lanes 0),
   kPcSlow / kRtSlow (ip - tb outside 2..251: counts of 252..257, 508..513),
   search counts of 256 and more (`while (c0 == kWinBytes)`, kPcEntry's
   `s_cmpk_eq_u32 t3, 0x100`).
E  the distance rule `cand + kMaxDistance >= pos` with equal bytes at
   distances 65,534..65,537 and 70,000: the general window's check and the
   re-test's, in the LDS-resident wide kernel (96 KiB), in k_lz4_encode_big
   (256 KiB) and, one far copy per block, in the smallest wide blocks (65,552
   and 65,568 bytes); the byU16 / byU32 boundary at 65,536..65,568 bytes.
   The third check, in the read-back window, is NOT reached: variant 128 is
   dispatched for 2-byte elements and byU16 blocks only, where the check is
   constant true, and a wide block takes the read-back search only when the
   launch finds the device's LDS atomics not lane-ordered, which they are on
   the MI355X.  The variant dispatch is byU16-only as well: a wide block runs
   the same kernel under every variant value, so the variants add nothing to
   the wide cases (they are set all the same, so that a later variant that
   does apply to wide blocks is run).

Each family runs in two block orders within a call (another block's record is
pending), under every variant of test_encoder_variant_all_element_sizes (for
element size 2 also 128, 8, 512, 2048: the read-back search, lane 0's
exchange, the general windows, the compiled compares), and once through the
host API; family A also through the batch API.  Comparisons are tobytes()
equality.
"""
import numpy as np
import pytest

from tests import search_cases as S
from tests.gpu_run import bs, run_case, torch, variant  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ALL_E = [0, 8192, 16384, 24576, 40960, 57344, 65536, 319488, 172032, 450560, 2793472, 3072000]
E2_ONLY = [128, 8, 512, 2048]


def variants(E):
    return ALL_E + (E2_ONLY if E == 2 else [])


def run_family(bs, torch, oracle, variant, blocks, E, be, block_arg=0, last=()):
    """The (equally long) blocks in two orders under every variant, each time
    with the shorter blocks of `last` behind them, then the host API."""
    last = list(last)
    a, want = run_case(bs, torch, oracle, variant, blocks + last, E, be, block_arg, variants=variants(E))
    again = blocks[::-1] + (last or blocks[1::2])
    run_case(bs, torch, oracle, variant, again, E, be, block_arg, variants=variants(E))
    variant(0)
    assert bs.compress_lz4(a, block_arg).tobytes() == want.tobytes()


def family_a(oracle, E):
    n = S.block_bytes(oracle, E)
    return [b for b, _ in S.catchup_cases(n)] + [b for b, _ in S.anchor_cases(n)] + [S.block_start_case(n)[0]]


def family_b(oracle, E):
    n = S.block_bytes(oracle, E)
    return [S.probe_cases(n)] + list(S.block_end_cases(n).values())


@pytest.mark.parametrize("E", [2, 4, 3])
def test_a_catch_up_lengths(bs, torch, oracle, variant, E):
    run_family(bs, torch, oracle, variant, family_a(oracle, E), E, oracle.default_block_size(E))


@pytest.mark.parametrize("E", [2, 4, 3])
def test_a_catch_up_to_the_block_start_32k(bs, torch, oracle, variant, E):
    n = S.block_bytes(oracle, E, 32768)
    blocks = [S.block_start_case(n)[0], S.block_start_case(n, seed=14)[0]]
    short = S.catchup_cases(S.block_bytes(oracle, E))[6][0]      # a short last block
    run_family(bs, torch, oracle, variant, blocks, E, n // E, n // E, last=[short])


@pytest.mark.parametrize("E", [2, 3])
def test_b_probe_schedule_and_block_end(bs, torch, oracle, variant, E):
    run_family(bs, torch, oracle, variant, family_b(oracle, E), E, oracle.default_block_size(E))


@pytest.mark.parametrize("E,n", [(1, 16), (1, 24), (1, 32), (1, 40), (2, 16), (2, 32), (3, 24), (4, 32)])
def test_b_blocks_around_the_minimum_length(bs, torch, oracle, variant, E, n):
    seen, unseen = S.tiny_cases(n)
    rnd = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    run_family(bs, torch, oracle, variant, [seen, unseen, rnd, seen, seen, unseen], E, n // E, n // E)


@pytest.mark.parametrize("E", [2, 3])
def test_c_window_traffic(bs, torch, oracle, variant, E):
    run_family(bs, torch, oracle, variant, S.window_cases(S.block_bytes(oracle, E)), E, oracle.default_block_size(E))


@pytest.mark.parametrize("E", [2, 3])
def test_d_count_window_edges(bs, torch, oracle, variant, E):
    run_family(bs, torch, oracle, variant, S.count_cases(S.block_bytes(oracle, E)), E, oracle.default_block_size(E))


@pytest.mark.parametrize("E,n", [(1, 98304), (3, 98304), (1, 262144), (3, 262152)])
def test_e_distance_rule(bs, torch, oracle, variant, E, n):
    run_family(bs, torch, oracle, variant, [S.far_case(n), S.boundary_case(n)], E, n // E, n // E)


@pytest.mark.parametrize("E,n", [(1, 65552), (3, 65568)])
def test_e_distance_rule_in_the_smallest_wide_block(bs, torch, oracle, variant, E, n):
    for retest in (False, True):
        for dists in ((65534, 65536), (65535, 65537)):      # at most three blocks per call
            blocks = [S.small_far_case(n, d, retest) for d in dists]
            run_family(bs, torch, oracle, variant, blocks, E, n // E, n // E)


@pytest.mark.parametrize("E,n", [(1, 65536), (1, 65544), (3, 65544), (1, 65552), (3, 65568)])
def test_e_table_type_boundary(bs, torch, oracle, variant, E, n):
    run_family(bs, torch, oracle, variant, [S.boundary_case(n), S.boundary_case(n, seed=57)], E, n // E, n // E)


@pytest.mark.parametrize("E,n", [(1, 65552), (3, 65568)])
def test_e_wide_blocks_then_a_short_byu16_block(bs, torch, oracle, variant, E, n):
    last = S.catchup_cases(S.block_bytes(oracle, E))[6][0]      # a catch-up of 65 bytes
    run_family(bs, torch, oracle, variant, [S.boundary_case(n), S.boundary_case(n, seed=57)], E, n // E, n // E,
               last=[last])


def test_a_batch_of_three_families(bs, torch, oracle, variant):
    be = oracle.default_block_size(2)
    n = be * 2
    shs = [np.concatenate(family_a(oracle, 2)),
           np.concatenate(S.window_cases(n) + S.count_cases(n) + [S.anchor_cases(n)[4][0][:1200]]),
           np.concatenate(family_b(oracle, 2)[:4] + family_a(oracle, 2)[3:9])]
    arrs = [oracle.bitunshuffle(sh.view(np.int16), be) for sh in shs]
    want = [oracle.compress_lz4(a, 0) for a in arrs]
    xs = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    for v in variants(2):
        variant(v)
        outs = bs.compress_lz4_batch_dev(xs, 0)
        for o, w in zip(outs, want):
            assert o.cpu().numpy().tobytes() == w.tobytes(), v

"""TEST INFRASTRUCTURE ONLY -- the inputs shared by tests/test_fast_model.py
(CPU) and tests/test_gpu_fast.py (GPU): the smallest shapes at which the fast
encoder can go wrong.  Every case is (id, raw bytes, elem_size, block_size)."""
import numpy as np

DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

# (E, n): full blocks + a 72-element partial block + a 5-element tail; two
# blocks + one group; E = 1; odd element sizes (staged transpose); E = 8;
# tail only; a block below LZ4's 13-byte minimum; nothing
SHAPES = [(2, 3 * 4096 + 77), (4, 2 * 2048 + 8), (1, 8192 + 16), (3, 2 * 2728 + 24),
          (12, 680 + 16), (8, 1024 * 2), (2, 5), (1, 8), (2, 0)]
KINDS = ["gen", "zeros", "random", "period3"]


def view_e(data, E):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    return data.view(DTYPES[E]) if E in DTYPES else data.view(np.dtype("V%d" % E))


def gen_bytes(oracle, nbytes, which):
    """nbytes of G1 int16 (which = 1) or G2 float32 (2) from element 0, seed 12345."""
    if which == 1:
        a = oracle.gen_g1((nbytes + 1) // 2, 0, 12345)
    else:
        a = oracle.gen_g2((nbytes + 3) // 4, 0, 12345)
    return a.view(np.uint8)[:nbytes].copy()


def data_bytes(oracle, kind, E, n):
    nbytes = E * n
    if kind == "gen":  # G2 for the float-like element sizes, G1 otherwise
        return gen_bytes(oracle, nbytes, 2 if E in (4, 8, 12) else 1)
    if kind == "zeros":
        return np.zeros(nbytes, dtype=np.uint8)
    if kind == "random":
        return np.random.default_rng(1000 * E + n).integers(0, 256, nbytes, dtype=np.uint8)
    if kind == "period3":  # a pattern of period 3 elements
        pat = np.random.default_rng(7).integers(0, 256, 3 * E, dtype=np.uint8)
        return np.resize(pat, nbytes).astype(np.uint8)
    raise ValueError(kind)


def many_sequences(oracle, nblocks=2):
    """int16 data whose bit-transposed 8 KiB blocks are 5-byte groups of equal
    bytes with different neighbours: every group is a 4-byte match at offset 1
    behind one literal, about 1,638 sequences per block."""
    L = 8192
    s = ((np.arange(nblocks * L) // 5 * 37) % 256).astype(np.uint8)
    return oracle.bitunshuffle(s.view(np.uint16), 4096).view(np.uint8).copy()


def cases(oracle):
    out = []
    for E, n in SHAPES:
        for kind in KINDS:
            out.append(("E%d_n%d_%s" % (E, n, kind), data_bytes(oracle, kind, E, n), E, 0))
    out.append(("many_sequences", many_sequences(oracle), 2, 0))
    # explicit block sizes: 16-byte blocks, 128-byte blocks, 2720-byte blocks
    out.append(("bs8", gen_bytes(oracle, 2 * 1237, 1), 2, 8))
    out.append(("bs64", gen_bytes(oracle, 2 * 1237, 1), 2, 64))
    out.append(("bs680", gen_bytes(oracle, 4 * (3 * 680 + 44), 2), 4, 680))
    out.append(("bs680_zeros", np.zeros(4 * (3 * 680 + 44), dtype=np.uint8), 4, 680))
    # blocks between 8 KiB and the 65,536-byte limit: the 8-slot LDS layout with
    # more than 256 bitmap words, the staged transpose past the register
    # transpose's size (and a 4104-element partial block), and at exactly
    # 65,536 bytes the largest LDS request and the longest possible run
    out.append(("bs16384", gen_bytes(oracle, 2 * (16384 + 4104 + 5), 1), 2, 16384))
    out.append(("bs32768", gen_bytes(oracle, 2 * (32768 + 72 + 3), 1), 2, 32768))
    out.append(("bs32768_zeros", np.zeros(2 * (32768 + 72 + 3), dtype=np.uint8), 2, 32768))
    out.append(("E4_bs16384", gen_bytes(oracle, 4 * (16384 + 16), 2), 4, 16384))
    return out


def big_block_case(oracle):
    """Blocks of 65,600 bytes: above the fast parse's limit, so the exact stream."""
    return ("E8_bs8200", gen_bytes(oracle, 8 * (2 * 8200 + 24), 1), 8, 8200)


def segmented_case(oracle):
    """65,541 blocks of 16 bytes + a tail (the encoder's segmented launches),
    made of 37 distinct blocks so that a model can cache payloads."""
    base = gen_bytes(oracle, 2 * 8 * 37, 1)
    n = (65536 + 5) * 8 + 3
    return ("segmented_bs8", np.resize(base, 2 * n).astype(np.uint8), 2, 8)


# the ratio table of the issue: (label, generator, E, default blocks)
RATIO_INPUTS = [("G1 int16", 1, 2, 64), ("G2 float32", 2, 4, 64), ("G1 bytes as E=3", 1, 3, 64),
                ("G2 bytes as E=12", 2, 12, 64), ("G1 bytes as E=1", 1, 1, 32),
                ("G2 bytes as E=8", 2, 8, 32)]


def ratio_input(oracle, gen, E, nblocks):
    n = nblocks * oracle.default_block_size(E)
    return view_e(gen_bytes(oracle, n * E, gen), E)

"""The fast encoder (csrc/lz4_fast.hip) on the crafted blocks of
tests/fast_craft.py, byte for byte against the numpy model of "fast parse v1"
(tests/fast_model.py).  tests/test_fast_craft.py proves on the CPU what every
block holds; here one call per shape family runs them through the kernel
instance the shape reaches:

  E2_bs4096   ek2/sreg   all four start registers
  E4_bs544    ek4/sreg   second register partly filled
  E1_bs384    ek1/sreg   one register, few lanes
  E3_bs2728   ek0/slot8  staged transpose, last word partial, P = 341
  E1_bs8200   ek1/slot8  257 words, P = 1025
  E8_bs1024   ek8/slot8
  E2_bs16384  ek2/slot8  32 KiB: more than 64 length bytes, several search windows
  tiny        E = 2, 4 with P = 1..8, 16: the merged offset sets
  partial     a last block with its own P (SREG: transposed straight from HBM)

A mismatch is reported as the first differing block's case, the model's
sequences around the difference and the kernel's, parsed from its payload.
Byte work: every comparison is exact."""
import numpy as np
import pytest

from tests import fast_cases, fast_craft, fast_model

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


def _records(stream, sizes):
    """[payload] per block of a framed stream, walked by its own length words
    (None from where it stops making sense)."""
    pos, out = 0, []
    for L in sizes:
        c = int.from_bytes(stream[pos:pos + 4].tobytes(), "big") if pos + 4 <= stream.size else -1
        if c < 0 or c > L + L // 255 + 16 or pos + 4 + c > stream.size:
            out += [None] * (len(sizes) - len(out))
            break
        out.append(stream[pos + 4:pos + 4 + c])
        pos += 4 + c
    return out


def explain(got, want, cases):
    """What differs: the first block whose record is not the model's."""
    sizes = [c.s.size for c in cases]
    for i, (g, w, c) in enumerate(zip(_records(got, sizes), _records(want, sizes), cases)):
        if g is None:
            return "block %d (%s): the kernel's record length is out of range" % (i, c.id)
        if g.tobytes() == w.tobytes():
            continue
        sg, sw = fast_craft.sequences(g), fast_craft.sequences(w)
        k = next((j for j, (a, b) in enumerate(zip(sg, sw)) if a != b), min(len(sg), len(sw)))
        pos = sum(ll + ml for ll, _, ml in sw[:k])
        byte = next((j for j, (a, b) in enumerate(zip(g.tolist(), w.tolist())) if a != b), min(g.size, w.size))
        if sg == sw:
            return ("block %d (%s): the sequences %r agree, a literal differs at payload byte %d (%d, model %d)"
                    % (i, c.id, sw, byte, g[byte], w[byte]))
        return ("block %d (%s, declared parse %r): sequence %d at block byte %d, payload byte %d (%d / %d payload "
                "bytes); (literals, offset, match) around it -- model %r, kernel %r"
                % (i, c.id, c.parse, k, pos, byte, g.size, w.size, sw[max(k - 2, 0):k + 3], sg[max(k - 2, 0):k + 3]))
    return "the records agree; stream lengths %d / %d (the tail?)" % (got.size, want.size)


def run_family(bs, torch, oracle, cases, m, last=None):
    """The family as one stream through the single-stream device entry: equal
    to the model, decoded back by the device and by the host oracle."""
    E = cases[0].E
    raw = fast_craft.stream(oracle, cases, m, last)
    arr = fast_cases.view_e(raw, E)
    want = fast_model.compress_lz4(oracle, arr, m)
    x = torch.from_numpy(raw).cuda()
    res = torch.full((1,), -0x5A5A5A5A, dtype=torch.int64, device="cuda")
    got_dev = bs.compress_lz4_dev(x, m, elem_size=E, mode="fast", result=res)
    got = got_dev.cpu().numpy()
    if got.tobytes() != want.tobytes():
        pytest.fail(explain(got, want, cases + ([last] if last else [])))
    assert int(res.item()) == want.size
    back = bs.decompress_lz4_dev(got_dev, (arr.size,), None, m, elem_size=E)
    assert back.cpu().numpy().tobytes() == raw.tobytes()
    assert oracle.decompress_lz4(got, arr.shape, arr.dtype, m).tobytes() == raw.tobytes()
    return raw, got


@pytest.mark.parametrize("name,E,m", fast_craft.SHAPES, ids=[s[0] for s in fast_craft.SHAPES])
def test_shape_family(bs, torch, oracle, name, E, m):
    cases = fast_craft.shape_cases(name, E, m)
    assert len(cases) > 40
    run_family(bs, torch, oracle, cases, m)
    run_family(bs, torch, oracle, cases[::-1], m)  # other neighbours, another block first


@pytest.mark.parametrize("E", [2, 4])
def test_tiny_blocks_offset_set_merging(bs, torch, oracle, E):
    for name, e, m in fast_craft.TINY:
        if e == E:
            cases = fast_craft.shape_cases(name, E, m)
            run_family(bs, torch, oracle, cases * 3, m)  # dozens of blocks per stream


@pytest.mark.parametrize("name,E,m,m_last", fast_craft.PARTIAL, ids=[s[0] for s in fast_craft.PARTIAL])
def test_partial_last_block_with_its_own_P(bs, torch, oracle, name, E, m, m_last):
    full, last = fast_craft.partial_cases(name, E, m, m_last)
    run_family(bs, torch, oracle, full, m, last)


def test_batch_call_equals_the_single_stream(bs, torch, oracle):
    """The E2_bs4096 family as three streams cut at block boundaries: the
    batch entry's records are the single-stream call's."""
    name, E, m = fast_craft.SHAPES[0]
    cases = fast_craft.shape_cases(name, E, m)
    _, single = run_family(bs, torch, oracle, cases, m)
    cuts = [0, 7, len(cases) - 20, len(cases)]
    parts = [cases[a:b] for a, b in zip(cuts, cuts[1:])]
    xs = [torch.from_numpy(fast_craft.stream(oracle, p, m)).view(torch.int16).cuda() for p in parts]
    outs = [o.cpu().numpy() for o in bs.compress_lz4_batch_dev(xs, m, mode="fast")]
    got = np.concatenate(outs)
    if got.tobytes() != single.tobytes():
        pytest.fail(explain(got, single, cases))
    for p, o in zip(parts, outs):
        arr = fast_craft.stream(oracle, p, m).view(np.int16)
        assert o.tobytes() == fast_model.compress_lz4(oracle, arr, m).tobytes()


def test_host_entry(bs, oracle):
    name, E, m = fast_craft.SHAPES[1]
    cases = fast_craft.shape_cases(name, E, m)
    arr = fast_craft.stream(oracle, cases, m).view(np.uint32)
    want = fast_model.compress_lz4(oracle, arr, m)
    got = bs.compress_lz4(arr, m, mode="fast")
    if got.tobytes() != want.tobytes():
        pytest.fail(explain(np.asarray(got), want, cases))
    assert bs.decompress_lz4(got, arr.shape, arr.dtype, m).tobytes() == arr.tobytes()

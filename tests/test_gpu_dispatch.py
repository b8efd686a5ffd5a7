"""GPU sweep of the kernel dispatch (bitshuffle_amd/csrc/dispatch.h): every
device entry point at every cell of tests/dispatch_cases.py -- element size x
block-byte class x pointer offsets -- against the CPU oracle (the numpy model
of the fast parse for mode="fast"), byte for byte.

Every pointer handed to the library is a slice of a larger buffer prefilled
with 0xA5, at least 64 canary bytes on each side: the canaries must be
untouched afterwards, and since the buffer is filled anew for every call a
store that never happened shows as 0xA5 in the payload, never as the stale
bytes of an earlier cell.  A test walks all its cells, collects every
mismatch with the path tests/dispatch_model.py names for it, and asserts that
the list is empty, so one wrong cell does not hide the rest.
"""
import ctypes

import numpy as np
import pytest

from tests import dispatch_cases as C
from tests import dispatch_model as M
from tests import fast_model

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


class Buf:
    """`nbytes` at `off` bytes into a 16-aligned allocation, inside canaries."""

    def __init__(self, torch, nbytes, off, data=None):
        self.lo = C.CANARY + off
        self.n = nbytes
        self.t = torch.full((self.lo + nbytes + C.CANARY + 16,), C.FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[self.lo:self.lo + nbytes]
        assert self.view.data_ptr() % 16 == off
        if data is not None:
            self.view.copy_(data)

    def canaries_ok(self, used=None):
        """Nothing outside the first `used` bytes of the payload was written."""
        used = self.n if used is None else used
        return bool((self.t[:self.lo] == C.FILL).all()) and bool((self.t[self.lo + used:] == C.FILL).all())

    def equals(self, want, n=None):
        n = want.size if n is None else n
        return self.view[:n].cpu().numpy().tobytes() == want.tobytes()


_EXPECTED = {}


def expected(oracle, torch, E, nbytes):
    """The three streams of cell (E, block bytes) and their expected bytes,
    computed once and shared by every test of the cell: raw input, exact
    stream, header offsets."""
    key = (E, nbytes)
    if key not in _EXPECTED:
        bsz = nbytes // E
        out = []
        for i, (name, nelem) in enumerate(C.streams(E, nbytes, three=True)):
            raw = C.stream_bytes(E, nbytes, 1000 * E + i, nelem)
            arr = C.view_e(raw, E)
            exact = oracle.compress_lz4(arr, bsz)
            nfull, last, _ = M.layout(nelem, bsz)
            nb = nfull + (1 if last else 0)
            out.append(dict(name=name, nelem=nelem, raw=raw, arr=arr, exact=exact, nb=nb,
                            offs=C.header_walk(exact, nb), d_raw=torch.from_numpy(raw).cuda(),
                            d_exact=torch.from_numpy(exact).cuda()))
        _EXPECTED[key] = out
    return _EXPECTED[key]


def single_streams(oracle, torch, E, nbytes):
    """The cell's streams for the single-stream calls (the batch calls take
    all three)."""
    return expected(oracle, torch, E, nbytes)[:len(C.streams(E, nbytes))]


_FAST_CACHE = {}


def fast_expected(oracle, torch, st, E, bsz):
    """mode="fast": the numpy model's stream; above kFastMaxBlockBytes the
    oracle's exact stream itself."""
    if bsz * E > M.FAST_MAX_BLOCK_BYTES:
        return st["exact"], st["offs"], st["d_exact"]
    if "fast" not in st:
        if len(_FAST_CACHE) > 64:
            _FAST_CACHE.clear()
        st["fast"] = fast_model.compress_lz4(oracle, st["arr"], bsz, cache=_FAST_CACHE)
        st["fast_offs"] = C.header_walk(st["fast"], st["nb"])
        st["d_fast"] = torch.from_numpy(st["fast"].copy()).cuda()
    return st["fast"], st["fast_offs"], st["d_fast"]


def _ids(cells):
    return ["E%d-%s" % (E, name) for E, name, _ in cells]


def _encode_decode_cell(bs, oracle, torch, E, nbytes, mode):
    bsz = nbytes // E
    bad = []
    for st in single_streams(oracle, torch, E, nbytes):
        nelem, nb = st["nelem"], st["nb"]
        if mode == "fast":
            want, want_offs, d_want = fast_expected(oracle, torch, st, E, bsz)
        else:
            want, want_offs, d_want = st["exact"], st["offs"], st["d_exact"]
        bound = bs.compress_lz4_bound(nelem, E, bsz)
        for oi, oo in C.OFFSETS:
            paths = (M.encode(E, bsz, nelem, oi, oo, fast=mode == "fast"), M.decode(E, bsz, nelem, oo, oi))
            where = (st["name"], oi, oo)
            src = Buf(torch, st["raw"].size, oi, st["d_raw"])
            out = Buf(torch, bound, oo)
            offs = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
            got = bs.compress_lz4_dev(src.view, bsz, out=out.view, offsets=offs, elem_size=E, mode=mode)
            if got.numel() != want.size or not out.equals(want):
                bad.append(where + ("encode bytes", paths[0]))
            if offs.cpu().tolist() != want_offs:
                bad.append(where + ("encode offsets", paths[0]))
            if not out.canaries_ok(bound) or not src.canaries_ok() or not src.equals(st["raw"]):
                bad.append(where + ("encode canaries", paths[0]))
            # decode: the stream at the output offset, the data at the data offset
            stream = Buf(torch, want.size, oo, d_want)
            index = torch.tensor(want_offs, dtype=torch.int64, device="cuda")
            for how, kw in (("index", dict(offsets=index)), ("rebuild", {})):
                back = Buf(torch, st["raw"].size, oi)
                try:
                    bs.decompress_lz4_dev(stream.view, (nelem,), None, bsz, out=back.view, elem_size=E, **kw)
                    ok = back.equals(st["raw"])
                except bs.BshufError as e:
                    ok = False
                    how += " error %r" % (e.args,)
                if not ok:
                    bad.append(where + ("decode bytes (%s)" % how, paths[1]))
                if not back.canaries_ok() or not stream.canaries_ok():
                    bad.append(where + ("decode canaries (%s)" % how, paths[1]))
    return bad


@pytest.mark.parametrize("E,name,nbytes", C.cells(), ids=_ids(C.cells()))
def test_exact_encode_and_decode(bs, oracle, torch, E, name, nbytes):
    """bshuf_compress_lz4_dev == the oracle's stream, its block offsets == a
    header walk; bshuf_decompress_lz4_dev of that stream, with the encoder's
    offsets and with the index rebuild, == the input."""
    bad = _encode_decode_cell(bs, oracle, torch, E, nbytes, "exact")
    assert not bad, bad


@pytest.mark.parametrize("E,name,nbytes", C.fast_cells(), ids=_ids(C.fast_cells()))
def test_fast_encode_and_decode(bs, oracle, torch, E, name, nbytes):
    """The same calls with mode="fast" == the numpy model of fast parse v1
    (above kFastMaxBlockBytes: the oracle's exact stream), and decode back."""
    bad = _encode_decode_cell(bs, oracle, torch, E, nbytes, "fast")
    assert not bad, bad


def _transpose_cell(bs, oracle, torch, E, bsz, raw, nelem):
    arr = C.view_e(raw, E)
    shuf = oracle.bitshuffle(arr, bsz).view(np.uint8).reshape(-1)
    d_raw, d_shuf = torch.from_numpy(raw).cuda(), torch.from_numpy(shuf).cuda()
    bad = []
    for oi, oo in C.OFFSETS:
        for what, fn, d_in, want in (("shuf", bs.lib.bshuf_bitshuffle_dev, d_raw, shuf),
                                     ("unshuf", bs.lib.bshuf_bitunshuffle_dev, d_shuf, raw)):
            src = Buf(torch, raw.size, oi, d_in)
            out = Buf(torch, raw.size, oo)
            r = fn(ctypes.c_void_p(src.view.data_ptr()), ctypes.c_void_p(out.view.data_ptr()), nelem, E, bsz,
                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            path = M.transpose(E, bsz, nelem, oi, oo, what)
            if r != raw.size or not out.equals(want):
                bad.append((what, oi, oo, "bytes", path))
            if not out.canaries_ok() or not src.canaries_ok():
                bad.append((what, oi, oo, "canaries", path))
    return bad


@pytest.mark.parametrize("E,name,nbytes", C.cells(), ids=_ids(C.cells()))
def test_transposes(bs, oracle, torch, E, name, nbytes):
    """bshuf_bitshuffle_dev / bshuf_bitunshuffle_dev == the oracle's."""
    st = single_streams(oracle, torch, E, nbytes)[0]
    bad = _transpose_cell(bs, oracle, torch, E, nbytes // E, st["raw"], st["nelem"])
    assert not bad, bad


@pytest.mark.parametrize("E", C.ELEM_SIZES)
def test_transposes_tile_boundary_inside_a_block(bs, oracle, torch, E):
    """More than 256 groups per block, P % 16 == 0 and != 0."""
    bad = []
    for name, bsz in C.transpose_extra_blocks():
        nelem = C.stream_elems(E, bsz * E)
        raw = C.stream_bytes(E, bsz * E, 77 + E, nelem)
        bad += [(name,) + b for b in _transpose_cell(bs, oracle, torch, E, bsz, raw, nelem)]
    assert not bad, bad


def _batch_cell(bs, oracle, torch, E, nbytes, mode):
    bsz = nbytes // E
    sts = expected(oracle, torch, E, nbytes)
    assert len(sts) == 3 and len({st["raw"].tobytes() for st in sts}) == 3
    bad = []
    for residues in C.BATCH_RESIDUES:
        wants = [fast_expected(oracle, torch, st, E, bsz) if mode == "fast" else
                 (st["exact"], st["offs"], st["d_exact"]) for st in sts]
        state, paths = M.encode_batch(E, bsz, [st["nelem"] for st in sts], residues, fast=mode == "fast")
        srcs = [Buf(torch, st["raw"].size, r, st["d_raw"]) for st, r in zip(sts, residues)]
        bounds = [bs.compress_lz4_bound(st["nelem"], E, bsz) for st in sts]
        outs = [Buf(torch, b, r) for b, r in zip(bounds, residues)]
        offs = torch.full((sum(st["nb"] for st in sts),), -1, dtype=torch.int64, device="cuda")
        got = bs.compress_lz4_batch_dev([s.view for s in srcs], bsz, outs=[o.view for o in outs], offsets=offs,
                                        elem_size=E, mode=mode)
        for i, (st, r) in enumerate(zip(sts, residues)):
            where = (residues, i, st["name"], state)
            if got[i].numel() != wants[i][0].size or not outs[i].equals(wants[i][0]):
                bad.append(where + ("batch encode bytes", paths[i]))
            if not outs[i].canaries_ok(bounds[i]) or not srcs[i].canaries_ok():
                bad.append(where + ("batch encode canaries", paths[i]))
            # ... and its single-stream result at the same pointers
            one = Buf(torch, bounds[i], r)
            g1 = bs.compress_lz4_dev(srcs[i].view, bsz, out=one.view, elem_size=E, mode=mode)
            if g1.numel() != got[i].numel() or not bool((one.view[:g1.numel()] == got[i]).all()):
                bad.append(where + ("batch != single stream", paths[i]))
        if offs.cpu().tolist() != [o for w in wants for o in w[1]]:
            bad.append((residues, state, "batch encode offsets", paths))
        dstate, dpaths = M.decode_batch(E, bsz, [st["nelem"] for st in sts], residues)
        streams = [Buf(torch, w[0].size, r, w[2]) for w, r in zip(wants, residues)]
        backs = [Buf(torch, st["raw"].size, r) for st, r in zip(sts, residues)]
        bs.decompress_lz4_batch_dev([s.view for s in streams], [(st["nelem"],) for st in sts], None, bsz,
                                    outs=[b.view for b in backs], elem_size=E)
        for i, st in enumerate(sts):
            where = (residues, i, st["name"], dstate)
            if not backs[i].equals(st["raw"]):
                bad.append(where + ("batch decode bytes", dpaths[i]))
            if not backs[i].canaries_ok() or not streams[i].canaries_ok():
                bad.append(where + ("batch decode canaries", dpaths[i]))
    return bad


@pytest.mark.parametrize("E,name,nbytes", C.cells(), ids=_ids(C.cells()))
def test_batch_exact(bs, oracle, torch, E, name, nbytes):
    """Three streams at pointer residues (0, 8, 1), (0, 8, 8) and (0, 0, 0)
    through the batch calls: each equals the oracle's stream and its
    single-stream result, and decodes to its input."""
    bad = _batch_cell(bs, oracle, torch, E, nbytes, "exact")
    assert not bad, bad


@pytest.mark.parametrize("E,name,nbytes", C.fast_cells(), ids=_ids(C.fast_cells()))
def test_batch_fast(bs, oracle, torch, E, name, nbytes):
    bad = _batch_cell(bs, oracle, torch, E, nbytes, "fast")
    assert not bad, bad


@pytest.mark.parametrize("E", C.RANGE_ELEM_SIZES)
def test_ranges_windows_and_sets(bs, oracle, torch, E):
    """Range lists whose direct pieces land at output residues 0, 8, 4 and
    odd, and one whose pieces off 16 are all 8-aligned (the second group staged:
    E = 2, 4, 8 as EK = 0; E = 1 by byte stores), with `out` shifted by 0, 8 and
    3; the same windows through the window decode of one stream and of a set."""
    bsz = C.RANGE_BLOCK
    nelem = 12 * bsz + 8 * 5 + C.TAIL_ELEMS
    raw = C.stream_bytes(E, bsz * E, 500 + E, nelem)
    raw2 = C.stream_bytes(E, bsz * E, 600 + E, nelem)
    d_streams = [torch.from_numpy(oracle.compress_lz4(C.view_e(r, E), bsz)).cuda() for r in (raw, raw2)]
    index = bs.api.block_index_dev(d_streams[0], nelem, E, bsz)
    bad = []
    for name, ranges in C.range_lists(E).items():
        want = np.concatenate([raw[s * E:(s + c) * E] for s, c in ranges])
        for shift in C.RANGE_OUT_SHIFTS:
            groups = M.range_groups(E, bsz, C.direct_residues(E, ranges, shift))
            for how, kw in (("index", dict(offsets=index)), ("rebuild", {})):
                out = Buf(torch, want.size, shift)
                bs.decompress_lz4_ranges_dev(d_streams[0], nelem, None, ranges, bsz, out=out.view, elem_size=E, **kw)
                if not out.equals(want) or not out.canaries_ok():
                    bad.append((name, shift, "ranges (%s)" % how, groups))
        # windows of two blocks at the direct ranges' starts and at odd ones
        window = 2 * bsz
        starts = [s for s, c in ranges if c == window] + [1, bsz + 3, nelem - window]
        want = np.concatenate([raw[s * E:(s + window) * E] for s in starts])
        d_starts = torch.tensor(starts, dtype=torch.int64, device="cuda")
        ids = [i % 2 for i in range(len(starts))]
        want_set = np.concatenate([(raw, raw2)[i][s * E:(s + window) * E] for i, s in zip(ids, starts)])
        sset = bs.lz4_stream_set_dev(d_streams, [nelem, nelem], E, bsz)
        d_ids = torch.tensor(ids, dtype=torch.int64, device="cuda")
        for shift in C.RANGE_OUT_SHIFTS:
            out = Buf(torch, want.size, shift)
            bs.decompress_lz4_windows_dev(d_streams[0], nelem, None, d_starts, window, bsz, out=out.view,
                                          elem_size=E)
            if not out.equals(want) or not out.canaries_ok():
                bad.append((name, shift, "windows", M.window_path(E, bsz)))
            out = Buf(torch, want.size, shift)
            bs.decompress_lz4_windows_set_dev(sset, None, d_ids, d_starts, window, out=out.view, elem_size=E)
            if not out.equals(want_set) or not out.canaries_ok():
                bad.append((name, shift, "window set", M.window_path(E, bsz)))
    assert not bad, bad

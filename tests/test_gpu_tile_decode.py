"""Tile decode (bshuf_decompress_lz4_tiles_dev, bshuf_decompress_lz4_tiles_set_dev):
K tiles of rows x cols elements, row r of tile i being elements [starts[i] + r *
pitch, ... + cols) of one stream or of stream ids[i] of a set, starts and ids
device tensors -- byte for byte against slices of the CPU oracle's decode of the
oracle's streams.

Every call writes into an output filled with 0xA5 that has 64 guard bytes in
front and behind, which must come back untouched -- as must the whole slice of a
tile that is not decoded.  Every case runs with block indexes supplied and with
indexes rebuilt (by the call, or by the set).  No tolerances: tobytes()
equality."""
import copy

import numpy as np
import pytest

from tests.test_gpu_range_decode import Stream, raw_bytes

pytestmark = pytest.mark.gpu

GUARD = 64


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


@pytest.fixture(scope="module")
def make(bs, torch, oracle):
    cache = {}

    def get(E, block, size, gen=1):
        key = (E, block, size, gen)
        if key not in cache:
            dt = np.dtype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}.get(E, "V%d" % E))
            data = raw_bytes(oracle, size * E, gen).view(dt)
            buf = oracle.compress_lz4(data, block)
            cache[key] = Stream(bs, torch, oracle, buf, size, E, block)
            assert cache[key].want.tobytes() == data.tobytes()
        return cache[key]
    return get


def run_blocks(W, b):
    return (W + b - 2) // b + 1


def tile_shape(rows, cols, pitch, b, nb):
    """(rg, G, Mg): the fewest blocks per tile, ties to the larger rg (tile_plan.h)."""
    best = None
    for rg in range(1, rows + 1):
        G = -(-rows // rg)
        Mg = min(run_blocks((rg - 1) * pitch + cols, b), nb)
        if best is None or G * Mg <= best[0]:
            best = (G * Mg, rg, G, Mg)
    return best[1:]


class Tiles:
    """Streams of one element and block size; calls over streams[0] alone (ids None)
    or over the set of them."""

    def __init__(self, bs, torch, streams, bufs=None):
        self.bs, self.torch, self.streams = bs, torch, streams
        self.E, self.block = streams[0].E, streams[0].block
        self.sizes = [st.size for st in streams]
        self.nb_max = max(st.nb for st in streams)
        self.bufs = [st.buf for st in streams] if bufs is None else bufs
        self._sets = {}

    def sset(self, supplied):
        if supplied not in self._sets:
            offs = [st.offs for st in self.streams] if supplied else None
            self._sets[supplied] = self.bs.lz4_stream_set_dev(self.bufs, self.sizes, self.E, self.block,
                                                              offsets=offs)
        return self._sets[supplied]

    def good(self, i, start, rows, cols, pitch, over_set):
        if not 0 <= i < len(self.streams):
            return False
        st = self.streams[i]
        span = (rows - 1) * pitch + cols
        if span > st.size or not 0 <= start <= st.size - span:
            return False
        return not over_set or st.nb >= tile_shape(rows, cols, pitch, self.block, self.nb_max)[2]

    def touches(self, start, rows, cols, pitch, block):
        """Whether an element of the tile lies in block `block` of its stream."""
        b = self.block
        return any(s // b <= block <= (s + cols - 1) // b for s in range(start, start + rows * pitch, pitch))

    def expected(self, ids, starts, rows, cols, pitch, status):
        """(K, rows * cols * E) bytes: the oracle's slices; 0xA5 where the tile is not written."""
        E = self.E
        tb = rows * cols * E
        exp = np.full((len(starts), tb), 0xA5, dtype=np.uint8)
        for k, (i, s) in enumerate(zip(ids, starts)):
            if status[k] == tb:
                w = self.streams[i].want
                exp[k] = np.concatenate([w[(s + r * pitch) * E:(s + r * pitch + cols) * E] for r in range(rows)])
        return exp

    def run(self, ids, starts, rows, cols, pitch, supplied=True, shift=0, sset=None, want_status=None,
            want_result=None):
        """One call, sync=False; checks the output, the guards, the statuses and the result."""
        torch, E = self.torch, self.E
        over_set = ids is not None
        if not isinstance(starts, torch.Tensor):
            starts = torch.tensor(list(starts), dtype=torch.int64, device="cuda")
        if over_set and not isinstance(ids, torch.Tensor):
            ids = torch.tensor(list(ids), dtype=torch.int64, device="cuda")
        K, tb = starts.numel(), rows * cols * E
        whole = torch.full((GUARD + shift + K * tb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        out = whole[GUARD + shift:GUARD + shift + K * tb]
        status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
        if over_set:
            o, res = self.bs.decompress_lz4_tiles_set_dev(self.sset(supplied) if sset is None else sset,
                                                          torch.uint8, ids, starts, rows, cols, pitch, out=out,
                                                          status=status, elem_size=E, sync=False)
        else:
            st = self.streams[0]
            o, res = self.bs.decompress_lz4_tiles_dev(self.bufs[0], st.size, torch.uint8, starts, rows, cols,
                                                      pitch, self.block, out=out, status=status, elem_size=E,
                                                      offsets=st.offs if supplied else None, sync=False)
        torch.cuda.synchronize()
        assert o is out
        hst = starts.cpu().tolist()
        hid = ids.cpu().tolist() if over_set else [0] * K
        if want_status is None:
            want_status = [tb if self.good(i, s, rows, cols, pitch, over_set) else -71 for i, s in zip(hid, hst)]
        assert status.cpu().tolist() == want_status
        if want_result is None:
            bad = [c for c in want_status if c < 0]
            want_result = K * tb if not bad else (-71 if -71 in bad else bad[-1])
        assert int(res.item()) == want_result
        got = whole.cpu().numpy()
        lo = GUARD + shift
        assert got[:lo].tobytes() == b"\xa5" * lo, "bytes in front of the tiles were written"
        assert got[lo + K * tb:].tobytes() == b"\xa5" * GUARD, "bytes behind the tiles were written"
        exp = self.expected(hid, hst, rows, cols, pitch, want_status)
        body = got[lo:lo + K * tb].reshape(K, tb)
        if body.tobytes() != exp.tobytes():
            t = np.nonzero((body != exp).any(axis=1))[0]
            raise AssertionError("tiles %s (ids %s, starts %s) of %d differ, %d x %d at pitch %d, E %d"
                                 % (t[:8].tolist(), [hid[i] for i in t[:8]], [hst[i] for i in t[:8]], K, rows,
                                    cols, pitch, E))
        return status, res

    def both(self, ids, starts, rows, cols, pitch, **kw):
        self.run(ids, starts, rows, cols, pitch, supplied=True, **kw)
        self.run(ids, starts, rows, cols, pitch, supplied=False, **kw)


B = 64
MAIN = 6 * B + 40 + 5      # six full blocks, a partial block of 40 and a 5-element tail
LONG = 12 * B + 40 + 5     # thirteen blocks


# ---- every start ---------------------------------------------------------------------

@pytest.mark.parametrize("E,size,rows,cols,pitch,shape", [
    (1, MAIN, 3, 8, 100, (3, 1, 5)),
    (2, MAIN, 3, 8, 100, (3, 1, 5)),
    (3, MAIN, 3, 8, 100, (3, 1, 5)),
    (4, MAIN, 3, 8, 100, (3, 1, 5)),
    (8, MAIN, 3, 8, 100, (3, 1, 5)),
    (12, MAIN, 3, 8, 100, (3, 1, 5)),
    (1, 10 * B + 40 + 5, 3, 8, 256, (1, 3, 2)),
    (2, 10 * B + 40 + 5, 3, 8, 256, (1, 3, 2)),
    (3, 10 * B + 40 + 5, 3, 8, 256, (1, 3, 2)),
    (2, LONG, 7, 8, 117, (2, 4, 3)),
    (3, LONG, 7, 8, 117, (2, 4, 3)),
])
def test_every_start(bs, torch, make, E, size, rows, cols, pitch, shape):
    """Every start from one before the first valid one to one behind the last, in one
    shuffled call: one run (rg = rows), a window per row (rg = 1), groups of two rows
    with a ragged last one.  (The second shape spans 520 elements, so its stream is
    the first one's with four more full blocks.)"""
    st = make(E, B, size, gen=1 if E != 4 else 2)
    T = Tiles(bs, torch, [st])
    assert tile_shape(rows, cols, pitch, B, st.nb) == shape
    span = (rows - 1) * pitch + cols
    starts = list(range(-1, size - span + 2))
    assert len(starts) > 40
    order = np.random.default_rng(size + E).permutation(len(starts))
    starts = [starts[k] for k in order]
    T.both(None, starts, rows, cols, pitch, want_result=-71)
    T.both([0] * len(starts), starts, rows, cols, pitch, want_result=-71)
    # no tile refused: the byte count
    T.both(None, [0, 1, size - span], rows, cols, pitch)


def test_tail(bs, torch, make):
    """Tiles whose last row ends in the verbatim tail, and a last row that is tail only."""
    for E in (2, 3):
        st = make(E, B, MAIN)
        T = Tiles(bs, torch, [st])
        covered = MAIN - 5
        for rows, cols, pitch in ((3, 8, 100), (3, 4, 100), (2, 5, 212), (1, 5, 5), (4, 3, 64)):
            span = (rows - 1) * pitch + cols
            last0 = (rows - 1) * pitch                           # the last row's offset in the tile
            starts = [MAIN - span - k for k in range(0, 6)]      # ending 0 .. 5 elements before the end
            ends = [s + span for s in starts]
            assert max(ends) == MAIN and sum(e > covered for e in ends) >= 4
            if cols <= 5:
                assert any(s + last0 >= covered for s in starts), "no tail-only last row"
            T.both(None, starts + [0], rows, cols, pitch)
            T.both([0] * len(starts), starts, rows, cols, pitch)


@pytest.mark.parametrize("shift", [1, 8])
def test_out_alignment(bs, torch, make, shift):
    for E, cols in ((2, 8), (3, 37), (1, 100), (8, 40)):
        st = make(E, B, LONG)
        T = Tiles(bs, torch, [st])
        starts = [0, 1, 7, 63, 64, 65, 130, LONG - (2 * 117 + cols)]
        T.both(None, starts, 3, cols, 117, shift=shift)
        T.both([0] * len(starts), starts, 3, cols, 117, shift=shift)


# ---- the gather's launcher paths ---------------------------------------------------------

@pytest.mark.parametrize("E,cols,lanes", [
    (2, 8, 16),        # 16-byte rows: single bytes
    (1, 31, 16),       # 31
    (2, 100, 16),      # 200-byte rows: 16-byte chunks by 16 lanes
    (2, 300, 16),      # a few hundred bytes: more than one chunk per lane
    (8, 128, 16),      # 1024: the last row length of 16 lanes
    (1, 1025, 64),     # the first of a wave per row
    (8, 256, 64),      # 2048: the last of them
    (2, 1025, 256),    # the first of a workgroup per row
    (8, 300, 256),     # 2400 bytes
    (12, 200, 256),
])
def test_gather_paths(bs, torch, make, E, cols, lanes):
    """Rows under 32 bytes, of a few hundred bytes and above 2 KiB: every number of lanes
    per row the launcher picks (16 up to 1 KiB, 64 up to 2 KiB, else 256), at its
    boundaries, with starts of every alignment against the staging area."""
    rb = cols * E
    assert lanes == (16 if rb <= 1024 else 64 if rb <= 2048 else 256)
    size = 70 * B + 40 + 5
    st = make(E, B, size, gen=1 if E != 8 else 2)
    T = Tiles(bs, torch, [st])
    rows, pitch = 5 if cols < 600 else 3, cols + 19
    span = (rows - 1) * pitch + cols
    assert span < size
    starts = [0, 1, 2, 3, 5, 8, 13, 16, 33, 64, size - span - 17, size - span]
    for shift in (0, 3):
        T.both(None, starts, rows, cols, pitch, shift=shift)
    T.run([0] * len(starts), starts, rows, cols, pitch)


def test_default_blocks_device_made_starts(bs, torch, make):
    """Crops of frames of 2048 int16 per row in the default 4096-element blocks, ids and
    corners drawn on the device; 300-element rows share blocks (one run per tile), and
    with a pitch of four blocks every row is a group of its own."""
    b = 4096
    sizes = [24 * 2048 + 1000 + 3, 20 * 2048, 31 * 2048 + 8]
    T = Tiles(bs, torch, [make(2, b, n) for n in sizes])
    K = 61
    for rows, cols, pitch, rg in ((16, 300, 2048, 16), (3, 300, 4 * b, 1)):
        assert tile_shape(rows, cols, pitch, b, T.nb_max)[0] == rg
        span = (rows - 1) * pitch + cols
        g = torch.Generator(device="cuda").manual_seed(5 + rows)
        room = torch.tensor([n - span + 1 for n in sizes], dtype=torch.int64, device="cuda")
        ids = torch.randint(0, 3, (K,), generator=g, device="cuda", dtype=torch.int64)
        starts = torch.randint(0, 2 ** 40, (K,), generator=g, device="cuda", dtype=torch.int64) % room[ids]
        for shift in (0, 1):
            T.both(ids, starts, rows, cols, pitch, shift=shift)
        T.both(None, starts % room[0], rows, cols, pitch)
        # a real dtype: (K, rows, cols) of it
        y = bs.decompress_lz4_tiles_set_dev(T.sset(True), torch.int16, ids, starts, rows, cols, pitch)
        assert y.dtype == torch.int16 and tuple(y.shape) == (K, rows, cols)
        exp = T.expected(ids.cpu().tolist(), starts.cpu().tolist(), rows, cols, pitch, [rows * cols * 2] * K)
        assert y.cpu().numpy().tobytes() == exp.tobytes()
        y = bs.decompress_lz4_tiles_dev(T.bufs[0], sizes[0], torch.int16, starts % room[0], rows, cols, pitch)
        exp = T.expected([0] * K, (starts % room[0]).cpu().tolist(), rows, cols, pitch, [rows * cols * 2] * K)
        assert tuple(y.shape) == (K, rows, cols) and y.cpu().numpy().tobytes() == exp.tobytes()


# ---- limits: a tile that is a window ---------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(1, 70), (5, 14), (1, 1), (70, 1)])
def test_one_span_tiles_are_windows(bs, torch, make, rows, cols):
    """pitch == cols (a tile that is one contiguous span) and rows == 1: output,
    statuses and result are decompress_lz4_windows_dev's of the same starts."""
    st = make(2, B, MAIN)
    window = rows * cols
    starts = [-1, 0, 5, B - 1, B, MAIN - window, MAIN - window + 1, 2 ** 62, 3 * B + 17]
    K, wb = len(starts), window * 2
    t = torch.tensor(starts, dtype=torch.int64, device="cuda")
    for supplied in (True, False):
        got = []
        for tiles in (False, True):
            whole = torch.full((GUARD + K * wb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            out = whole[GUARD:GUARD + K * wb]
            status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
            kw = dict(out=out, status=status, elem_size=2, sync=False, offsets=st.offs if supplied else None)
            if tiles:
                _, res = bs.decompress_lz4_tiles_dev(st.buf, MAIN, torch.uint8, t, rows, cols, cols, B, **kw)
            else:
                _, res = bs.decompress_lz4_windows_dev(st.buf, MAIN, torch.uint8, t, window, B, **kw)
            torch.cuda.synchronize()
            got.append((whole.cpu().numpy().tobytes(), status.cpu().tolist(), int(res.item())))
        win, til = got
        assert win[1] == til[1] and win[2] == til[2] == -71
        assert win[0] == til[0]
        assert win[1].count(wb) == K - 3 and win[1].count(-71) == 3


# ---- sets ------------------------------------------------------------------------------

SMALL = [6 * B + 40 + 5,    # seven blocks and a tail
         4 * B,             # four blocks, no tail
         5,                 # tail only
         12 * B + 7,
         B + 24]            # a full and a partial block


@pytest.mark.parametrize("E", [2, 3])
def test_sets_of_streams_of_different_sizes(bs, torch, make, E):
    T = Tiles(bs, torch, [make(E, B, n) for n in SMALL])
    assert [st.nb for st in T.streams] == [7, 4, 0, 12, 2]
    for supplied in (True, False):
        assert T.sset(supplied).status.cpu().tolist() == [0] * 5
    for rows, cols, pitch in ((3, 8, 100), (3, 8, 256), (2, 3, 20), (1, 5, 5)):
        rg, G, Mg = tile_shape(rows, cols, pitch, B, T.nb_max)
        span = (rows - 1) * pitch + cols
        ids, starts = [], []
        for i, st in enumerate(T.streams):
            if st.size >= span and st.nb >= Mg:
                for s in sorted({0, 1, (st.size - span) // 2, st.size - span - 1, st.size - span} - {-1}):
                    ids.append(i)
                    starts.append(s)
            for s in (-1, 0, st.size - span + 1):
                ids.append(i)
                starts.append(s)
        for i in (-1, 5, 2 ** 40, -2 ** 63):            # ids outside the set
            ids.append(i)
            starts.append(0)
        order = np.random.default_rng(rows * 7 + cols).permutation(len(ids))
        ids, starts = [ids[k] for k in order], [starts[k] for k in order]
        want = [rows * cols * E if T.good(i, s, rows, cols, pitch, True) else -71 for i, s in zip(ids, starts)]
        assert want.count(-71) >= 4 + 2 * 5 and want.count(rows * cols * E) >= 6
        T.both(ids, starts, rows, cols, pitch, want_status=want, want_result=-71)


def test_stream_with_fewer_blocks_than_a_group(bs, torch, make):
    """(3, 8, 100) decodes five blocks per tile: the stream of four blocks that holds
    the span takes no such tile (-71, its slice untouched), its neighbours do."""
    T = Tiles(bs, torch, [make(2, B, n) for n in SMALL])
    assert tile_shape(3, 8, 100, B, T.nb_max) == (3, 1, 5) and SMALL[1] >= 208 and T.streams[1].nb == 4
    T.both([0, 1, 3, 1], [0, 0, 300, 48], 3, 8, 100, want_status=[48, -71, 48, -71], want_result=-71)
    # alone, that stream takes the tile
    one = Tiles(bs, torch, [T.streams[1]])
    one.both(None, [0, 48], 3, 8, 100)
    one.both([0, 0], [0, 48], 3, 8, 100)


def test_mismatched_set_header_touches_nothing(bs, torch, make):
    T = Tiles(bs, torch, [make(2, B, n) for n in (SMALL[0], SMALL[3], 5 * B)])
    ids, starts = [0, 1, 2, 1], [0, 100, 17, 12 * B + 7 - 208]
    for rows, cols, pitch in ((3, 8, 100), (3, 8, 256)):
        for supplied in (True, False):
            T.run(ids, starts, rows, cols, pitch, supplied=supplied)
            for field, value in (("count", 4), ("count", 2), ("max_size", 13 * B + 7), ("max_size", 9 * B),
                                 ("block_size", 2 * B), ("block_size", 8)):
                other = copy.copy(T.sset(supplied))
                setattr(other, field, value)
                T.run(ids, starts, rows, cols, pitch, sset=other, want_status=[-71] * 4, want_result=-71)


# ---- corrupt blocks -----------------------------------------------------------------------

def _hurt(torch, st, block):
    bad = st.buf.clone()
    o = int(st.offs[block].item())
    bad[o:o + 4] = torch.tensor([0x7F, 0xFF, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")
    return bad


@pytest.mark.parametrize("block", [2, 3])
def test_corruption_fails_exactly_the_tiles_that_hold_the_block(bs, torch, make, block):
    """(3, 8, 100) at start 0 has its rows in blocks 0, 1 and 3; block 2 lies between
    them and is decoded with them.  With the index supplied, destroying block 2's
    header leaves that tile good; destroying block 3's gives it that block's code and
    NONE of its rows is written, also not those of blocks 0 and 1.  The other tiles of
    the call fail exactly when one of their rows holds an element of the block."""
    rows, cols, pitch = 3, 8, 100
    tb = rows * cols * 2
    st = make(2, B, MAIN)
    other = make(2, B, LONG)
    bad = _hurt(torch, st, block)
    with pytest.raises(bs.BshufError) as whole:
        bs.decompress_lz4_dev(bad, (st.size,), torch.int16, B, offsets=st.offs)
    code = whole.value.args[1]
    assert code < 0
    T = Tiles(bs, torch, [st, other], bufs=[bad, other.buf])
    # blocks: 0,1,3  0,2,4  2,4,5   1,3,4+5  3,4,6 (partial)  1,2,4  0,1,3
    starts = [0, 56, 2 * B + 40, B + 50, 3 * B + 20, B + 10, 5]
    touch = [T.touches(s, rows, cols, pitch, block) for s in starts]
    assert touch[0] == (block == 3) and True in touch[1:] and False in touch[1:]
    want = [code if t else tb for t in touch]
    last = [c for c in want if c < 0]
    # one stream, index supplied
    T.run(None, starts, rows, cols, pitch, supplied=True, want_status=want, want_result=last[-1] if last else None)
    # ... rebuilt by the call: the records do not tile the stream
    t = torch.tensor(starts, dtype=torch.int64, device="cuda")
    _, res = bs.decompress_lz4_tiles_dev(bad, st.size, torch.int16, t, rows, cols, pitch, B, sync=False)
    torch.cuda.synchronize()
    assert int(res.item()) == -91
    # over a set, with tiles at the same starts in a stream that is whole
    ids, sts, swant, want91 = [], [], [], []
    for s, c in zip(starts, want):
        ids += [0, 1]
        sts += [s, s]
        swant += [c, tb]
        want91 += [-91, tb]
    assert T.sset(True).status.cpu().tolist() == [0, 0]
    assert T.sset(False).status.cpu().tolist() == [-91, 0]
    T.run(ids, sts, rows, cols, pitch, supplied=True, want_status=swant)
    T.run(ids, sts, rows, cols, pitch, supplied=False, want_status=want91, want_result=-91)
    # no failing tile: the byte count
    ok = [k for k in range(len(ids)) if swant[k] == tb]
    T.run([ids[k] for k in ok], [sts[k] for k in ok], rows, cols, pitch, supplied=True)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_tiles_dev(bad, st.size, torch.int16, t, rows, cols, pitch, B, offsets=st.offs)
    assert e.value.args[1] == code


def test_group_of_its_own_is_not_failed_by_a_neighbour(bs, torch, make):
    """rg = 1: a tile of three groups fails through the one group whose row holds the
    block, and is still not written at all."""
    rows, cols, pitch = 3, 8, 256
    tb = rows * cols * 2
    st = make(2, B, 10 * B + 40 + 5)
    bad = _hurt(torch, st, 4)                  # elements [256, 320)
    with pytest.raises(bs.BshufError) as whole:
        bs.decompress_lz4_dev(bad, (st.size,), torch.int16, B, offsets=st.offs)
    code = whole.value.args[1]
    T = Tiles(bs, torch, [st], bufs=[bad])
    starts = [0, 1, 60, 64, 130, 165]          # row 1 at 256 + start: block 4 up to start 63
    want = [code if T.touches(s, rows, cols, pitch, 4) else tb for s in starts]
    assert want == [code, code, code, tb, tb, tb]
    T.run(None, starts, rows, cols, pitch, supplied=True, want_status=want, want_result=code)
    T.run([0] * 6, starts, rows, cols, pitch, supplied=True, want_status=want, want_result=code)


# ---- the host side ---------------------------------------------------------------------

def test_host_refusals_zero_shapes_and_argument_errors(bs, torch, make):
    st = make(2, B, MAIN)
    T = Tiles(bs, torch, [st, make(2, B, LONG)])
    starts = torch.tensor([3, 100, 7], dtype=torch.int64, device="cuda")
    ids = torch.tensor([0, 1, 1], dtype=torch.int64, device="cuda")
    sset = T.sset(True)

    def one(rows, cols, pitch, **kw):
        return bs.decompress_lz4_tiles_dev(st.buf, MAIN, torch.int16, starts, rows, cols, pitch, B,
                                           offsets=st.offs, **kw)

    def over(rows, cols, pitch, **kw):
        return bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, starts, rows, cols, pitch, **kw)

    for f, size in ((one, MAIN), (over, LONG)):
        out = torch.full((3, 3, 8), 0x5A5A, dtype=torch.int16, device="cuda")
        for rows, cols, pitch in ((3, 8, 7), (3, 8, size), (2, size, size), (1, size + 1, size + 1)):
            with pytest.raises(bs.BshufError) as e:     # pitch < cols; span > size
                f(rows, cols, pitch, out=out if rows * cols == 24 else None)
            assert e.value.args[1] == -71, (rows, cols, pitch)
        assert (out == 0x5A5A).all()
        # zero tiles, rows or cols: result 0
        for K, rows, cols in ((0, 3, 8), (3, 0, 8), (3, 3, 0)):
            if f is one:
                o, res = bs.decompress_lz4_tiles_dev(st.buf, MAIN, torch.int16, starts[:K], rows, cols, 100, B,
                                                     sync=False)
            else:
                o, res = bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids[:K], starts[:K], rows, cols, 100,
                                                         sync=False)
            torch.cuda.synchronize()
            assert int(res.item()) == 0 and tuple(o.shape) == (K, rows, cols)
    for wrong in (starts.cpu(), starts.to(torch.int32), torch.stack([starts, starts], 1)[:, 0], starts.tolist()):
        with pytest.raises(ValueError):
            bs.decompress_lz4_tiles_dev(st.buf, MAIN, torch.int16, wrong, 3, 8, 100, B)
        with pytest.raises(ValueError):
            bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, wrong, 3, 8, 100)
        with pytest.raises(ValueError):
            bs.decompress_lz4_tiles_set_dev(sset, torch.int16, wrong, starts, 3, 8, 100)
    with pytest.raises(ValueError):
        bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids[:2], starts, 3, 8, 100)
    with pytest.raises(ValueError):                     # out too small
        one(3, 8, 100, out=torch.empty((3, 3, 7), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):                     # the set's element size
        bs.decompress_lz4_tiles_set_dev(sset, torch.int32, ids, starts, 3, 8, 100)


def test_caller_workspace_of_the_reported_size(bs, torch, make):
    """A caller workspace of exactly the reported size works, one byte less or a
    misaligned one is refused; the size is a function of the shape (no starts go in)."""
    st = make(2, B, LONG)
    T = Tiles(bs, torch, [st, make(2, B, LONG + B)])
    starts = torch.tensor([3, 100, 7, LONG - 710], dtype=torch.int64, device="cuda")
    ids = torch.tensor([0, 1, 1, 0], dtype=torch.int64, device="cuda")
    hid, hst = ids.tolist(), starts.tolist()
    for rows, cols, pitch in ((3, 8, 100), (3, 8, 256), (7, 8, 117)):
        tb = rows * cols * 2
        for supplied in (True, False):
            sset = T.sset(supplied)
            offs = st.offs if supplied else None
            n = int(bs.lib.bshuf_decompress_lz4_tiles_set_dev_workspace(LONG + B, 2, B, 4, rows, cols, pitch))
            n1 = int(bs.lib.bshuf_decompress_lz4_tiles_dev_workspace(st.buf.numel(), LONG, 2, B, 4, rows, cols,
                                                                     pitch))
            ws = bs.decompress_lz4_tiles_set_workspace(sset, 4, rows, cols, pitch)
            ws1 = bs.decompress_lz4_tiles_workspace(st.buf.numel(), LONG, 2, 4, rows, cols, pitch, B)
            assert ws.numel() == n and n % 256 == 0 and ws.data_ptr() % 256 == 0
            assert ws1.numel() == n1 and n1 % 256 == 0 and ws1.data_ptr() % 256 == 0
            y = bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, starts, rows, cols, pitch, workspace=ws)
            assert y.cpu().numpy().tobytes() == T.expected(hid, hst, rows, cols, pitch, [tb] * 4).tobytes()
            y = bs.decompress_lz4_tiles_dev(st.buf, LONG, torch.int16, starts, rows, cols, pitch, B,
                                            workspace=ws1, offsets=offs)
            assert y.cpu().numpy().tobytes() == T.expected([0] * 4, hst, rows, cols, pitch, [tb] * 4).tobytes()
            big = torch.empty(max(n, n1) + 512, dtype=torch.uint8, device="cuda")
            for short in (ws[:n - 1], big[16:16 + n]):
                with pytest.raises(bs.BshufError) as e:
                    bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, starts, rows, cols, pitch,
                                                    workspace=short)
                assert e.value.args[1] == -71
            for short in (ws1[:n1 - 1], big[16:16 + n1]):
                with pytest.raises(bs.BshufError) as e:
                    bs.decompress_lz4_tiles_dev(st.buf, LONG, torch.int16, starts, rows, cols, pitch, B,
                                                workspace=short, offsets=offs)
                assert e.value.args[1] == -71


def test_nothing_reaches_the_host(bs, torch, make, monkeypatch):
    b = 4096
    sizes = [24 * 2048 + 1000 + 3, 20 * 2048, 31 * 2048 + 8]
    T = Tiles(bs, torch, [make(2, b, n) for n in sizes])
    rows, cols, pitch = 8, 100, 2048
    ids = torch.tensor([0, 2, 0, 1], dtype=torch.int64, device="cuda")
    starts = torch.tensor([0, b - 1, 16 * 2048 + 900, 17], dtype=torch.int64, device="cuda")
    out = torch.full((4, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
    out1 = torch.full((4, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
    sets = [T.sset(True), T.sset(False)]
    st = T.streams[0]
    torch.cuda.synchronize()
    seen = []

    def spy(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **kw):
            seen.append((name, self))
            return orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("cpu", "item", "tolist"):
        spy(name)
    for sset in sets:
        o, res = bs.decompress_lz4_tiles_set_dev(sset, torch.int16, ids, starts, rows, cols, pitch, out=out,
                                                 sync=False)
    for offs in (st.offs, None):
        o1, res1 = bs.decompress_lz4_tiles_dev(st.buf, st.size, torch.int16, starts, rows, cols, pitch, b,
                                               out=out1, offsets=offs, sync=False)
    calls = list(seen)
    monkeypatch.undo()
    assert not calls, "a sync=False call read a tensor on the host: %s" % [n for n, _ in calls]
    torch.cuda.synchronize()
    tb = rows * cols * 2
    assert int(res.item()) == int(res1.item()) == 4 * tb
    exp = T.expected(ids.tolist(), starts.tolist(), rows, cols, pitch, [tb] * 4)
    assert out.cpu().numpy().tobytes() == exp.tobytes()
    exp = T.expected([0] * 4, starts.tolist(), rows, cols, pitch, [tb] * 4)
    assert out1.cpu().numpy().tobytes() == exp.tobytes()


@pytest.mark.parametrize("over_set", [False, True])
def test_capture_and_replay(bs, torch, make, over_set):
    """One captured call, replayed with other starts (and ids) in the same tensors."""
    b = 4096
    sizes = [24 * 2048 + 1000 + 3, 22 * 2048 + 24 + 5, 31 * 2048 + 8]
    T = Tiles(bs, torch, [make(2, b, n) for n in sizes])
    K, rows, cols, pitch = 32, 8, 300, 2048
    span = (rows - 1) * pitch + cols
    tb = rows * cols * 2
    nstream = 3 if over_set else 1
    plans = [
        ([(i * 7) % nstream for i in range(K)], lambda k, i: (k % 3) * b),                   # block-aligned
        ([(i * 5 + 1) % nstream for i in range(K)], lambda k, i: b - 1 + (k % 2) * 2048),    # straddling
        ([i % min(nstream, 2) for i in range(K)], lambda k, i: sizes[i] - span - (k % 3)),   # partial block, tail
    ]
    sets = [(ids, [f(k, i) for k, i in enumerate(ids)]) for ids, f in plans]
    assert all(T.good(i, s, rows, cols, pitch, over_set) for ids, ss in sets for i, s in zip(ids, ss))
    assert all(s + span > sizes[i] - sizes[i] % 8 for i, s in zip(*sets[2]))
    ids = torch.tensor([i % nstream for i in range(K)], dtype=torch.int64, device="cuda")
    starts = torch.tensor([5 + i for i in range(K)], dtype=torch.int64, device="cuda")
    out = torch.full((K, tb), 0xA5, dtype=torch.uint8, device="cuda")
    sset = T.sset(True)
    st = T.streams[0]
    if over_set:
        ws = bs.decompress_lz4_tiles_set_workspace(sset, K, rows, cols, pitch)
    else:
        ws = bs.decompress_lz4_tiles_workspace(st.buf.numel(), st.size, 2, K, rows, cols, pitch, b)
    result = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    news = [(torch.tensor(i, dtype=torch.int64, device="cuda"), torch.tensor(s, dtype=torch.int64, device="cuda"))
            for i, s in sets]
    torch.cuda.synchronize()

    def call():
        kw = dict(out=out, workspace=ws, result=result, status=status, elem_size=2, sync=False)
        if over_set:
            bs.decompress_lz4_tiles_set_dev(sset, torch.uint8, ids, starts, rows, cols, pitch, **kw)
        else:
            bs.decompress_lz4_tiles_dev(st.buf, st.size, torch.uint8, starts, rows, cols, pitch, b,
                                        offsets=st.offs, **kw)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    assert int(result.item()) == K * tb
    assert out.cpu().numpy().tobytes() == T.expected(ids.tolist(), starts.tolist(), rows, cols, pitch,
                                                     [tb] * K).tobytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    for (hid, hst), (ni, ns) in zip(sets, news):
        ids.copy_(ni)
        starts.copy_(ns)
        out.fill_(0xA5)
        result.zero_()
        status.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(result.item()) == K * tb
        assert status.cpu().tolist() == [tb] * K
        assert out.cpu().numpy().tobytes() == T.expected(hid, hst, rows, cols, pitch, [tb] * K).tobytes()

"""Every capturable device entry point, captured into a hipGraph in Global
mode and REPLAYED: bitshuffle.h promises that a *_dev call with a caller
workspace allocates nothing, never waits on the host and "can be captured into
a hipGraph"; what a replay needs beyond a first run is that every piece of
state -- ticket counters, foot[nb], the index rebuild's chunk counts, the
`bad` words, uploaded tables -- is set again by stream-ordered work of the
graph itself.

Each case (tests/hip_graph.py does the capture):
  1. buffers from torch, outside the capture: the output between 64-byte
     canaries of 0xA5, a workspace of exactly *_workspace() bytes, result and
     status words;
  2. one uncaptured call on the stream, compared byte-exact (the first encode
     of a process allocates: it must not be the captured one);
  3. the capture: the call returns what it returns uncaptured, the graph has
     only kernel, memcpy and memset nodes and is ONE LINEAR CHAIN;
  4. three replays with other contents written in place into the same input,
     the output refilled with 0xA5, the result words set to a sentinel and the
     whole workspace filled with 0x00, 0xFF and random bytes in turn: output,
     result words, canaries and block offsets byte-exact against the oracle;
  5. a back-to-back pair: replay, a stream-ordered copy of the next input,
     replay, with no host synchronisation between them.

Replay contents of one byte size: A oracle.gen_g1, B zeros, C random bytes --
their three streams have three different lengths (asserted), so a replay that
kept the first run's length fails.  Entries that are told the stream's length
by the HOST and rebuild the index (records must tile in_nbytes exactly: the
decode without offsets, the index, ranges without offsets, the batch decode,
the stream set) can only replay streams of one length: theirs are A with its
full blocks rotated (rot_contents), three distinct streams of one length with
other header offsets.  Varying lengths with a rebuilt index go through the
device-held length entries (_dlen).  The D2 decoy stream of
tests/index_model.py is not replayed in S1's graph: it is 50 blocks of 8 KiB
of 1-, 4- or 12-byte elements, and a graph is captured for one (size,
elem_size, block_size).

Shapes: S1 int16 / 4096 (register path; full blocks, a partial one, a raw
tail), S2 3-byte elements / default block (staged path), S3 uint8 / 64 with
both pointers at 8 mod 16 (byte stores), S4 4-byte elements with a block above
max_device_block_bytes() (global-memory path), S5 65,537 blocks of 128 bytes
(where the pipelined encode starts; under capture it must stay one chain),
S6 9,301 blocks of 64 bytes (more blocks than a persistent launch has waves,
so that tickets decide who takes a block; with 1 << 25 only).
Cases on S1 are captured a second time with bshuf_set_variant(1 << 25)
(tickets in every launch) set while capturing and cleared before the replays.
"""
import ctypes

import numpy as np
import pytest

from tests import dispatch_cases as C
from tests import dispatch_model as M
from tests import fast_model
from tests import hip_graph as H

pytestmark = pytest.mark.gpu

TICKETS = 1 << 25       # bshuf_set_variant bit: tickets in both kernels at every block size
SENTINEL = -0x5A5A5A5A5A5A5A5B
FILL = 0xA5
CANARY = 64
WS_FILLS = (0x00, 0xFF, "random")
VARIANTS = pytest.mark.parametrize("variant", [0, TICKETS], ids=["default", "tickets"])


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
def gs(torch):
    g = H.GraphStream()
    yield g
    g.close()


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- shapes and their replay contents ------------------------------------------
class Shape:
    def __init__(self, name, E, block, n, shift=0):
        self.name, self.E, self.block, self.n, self.shift = name, E, block, n, shift
        self.bsz = block or M.default_block_size(E)     # `block` 0: the library's default
        self.nbytes = n * E
        self.nfull = n // self.bsz
        self.nb = self.nfull + (1 if (n % self.bsz) // 8 else 0)


S4_BLOCK = C.above(M.max_device_block_bytes(), 4) // 4
S1 = Shape("S1", 2, 4096, 5 * 4096 + 1000 + 3)
S2 = Shape("S2", 3, 0, 3 * M.default_block_size(3) + 1000 + 5)
S3 = Shape("S3", 1, 64, 37 * 64 + 40 + 3, shift=8)
S4 = Shape("S4", 4, S4_BLOCK, C.stream_elems(4, S4_BLOCK * 4, nfull=2))
S5 = Shape("S5", 2, 64, 65536 * 64 + 40 + 5)
# more than twice the 4,608 waves a persistent launch can hold: most blocks are
# drawn from the ticket counters (with 1 << 25; 64-byte blocks are scheduled
# statically otherwise), so counters that a replay did not zero lose blocks
S6 = Shape("S6", 1, 64, 9300 * 64 + 40 + 3)
SHAPES = {s.name: s for s in (S1, S2, S3, S4, S5, S6)}


def abc_contents(oracle, nbytes, seed=0):
    """A, B, C of `nbytes` bytes: G1, zeros, random."""
    a = oracle.gen_g1(nbytes // 2 + 1, seed=12345 + seed).view(np.uint8)[:nbytes].copy()
    c = np.random.default_rng(4242 + seed).integers(0, 256, nbytes, dtype=np.uint8)
    return [a, np.zeros(nbytes, dtype=np.uint8), c]


def rot_contents(oracle, nbytes, E, bsz, seed=0):
    """Three distinct contents whose streams are equally long: G1 with its full
    blocks rotated by 0, 1, 2 (the same records in another order).  With two
    full blocks (a rotation by 2 is none) the second block is random bytes:
    G R, R G, and R' G with other random bytes (literal-only records of one
    length); with fewer than two, random bytes of three seeds."""
    nfull, n = nbytes // (bsz * E), bsz * E

    def rnd(k):
        return np.random.default_rng(99 + 7 * seed + k)

    if nfull < 2:
        return [rnd(k).integers(0, 256, nbytes, dtype=np.uint8) for k in range(3)]
    a = abc_contents(oracle, nbytes, seed)[0]
    if nfull == 2:
        a[n:2 * n] = rnd(0).integers(0, 256, n, dtype=np.uint8)
    out = []
    for k in range(3):
        r = a.copy()
        r[:nfull * n] = np.roll(a[:nfull * n].reshape(nfull, n), k if nfull > 2 else min(k, 1), axis=0).reshape(-1)
        if nfull == 2 and k == 2:
            r[:n] = rnd(1).integers(0, 256, n, dtype=np.uint8)
        out.append(r)
    return out


def all_differ(vs):
    return len({v.stream.tobytes() for v in vs}) == len(vs) and len({v.raw.tobytes() for v in vs}) == len(vs)


class Var:
    """One replay content of a shape: raw bytes, stream, header offsets, on
    the host and staged on the device."""

    def __init__(self, oracle, torch, raw, E, bsz, nb, fast=False):
        self.raw = raw
        arr = C.view_e(raw, E)
        if fast:
            self.stream = fast_model.compress_lz4(oracle, arr, bsz)
        else:
            self.stream = oracle.compress_lz4(arr, bsz) if raw.size else np.zeros(0, dtype=np.uint8)
        self.offs = C.header_walk(self.stream, nb)
        self.d_raw = torch.from_numpy(raw.copy()).cuda()
        self.d_stream = torch.from_numpy(self.stream.copy()).cuda()
        self.d_offs = torch.tensor(self.offs, dtype=torch.int64, device="cuda")
        self.d_len = torch.tensor([self.stream.size], dtype=torch.int64, device="cuda")


_VARS = {}


def variants_of(oracle, torch, sh, family, fast=False):
    """The three replay contents of shape `sh`, built once: family "abc"
    (three stream lengths) or "rot" (one length, moving headers)."""
    key = (sh.name, family, fast)
    if key not in _VARS:
        raws = abc_contents(oracle, sh.nbytes) if family == "abc" else rot_contents(oracle, sh.nbytes, sh.E, sh.bsz)
        vs = [Var(oracle, torch, r, sh.E, sh.bsz, sh.nb, fast) for r in raws]
        lens = [v.stream.size for v in vs]
        if family == "abc":
            assert len(set(lens)) == 3, "A, B, C must give three stream lengths: %r" % lens
        else:
            assert len(set(lens)) == 1, lens
            assert vs[0].offs != vs[1].offs
        assert all_differ(vs)
        _VARS[key] = vs
    return _VARS[key]


# ---- the rig: buffers of a case, and how every case is driven ---------------------
class Guarded:
    """`nbytes` at `shift` mod 16, between canaries of 0xA5."""

    def __init__(self, torch, nbytes, shift=0):
        self.lo, self.n = CANARY + shift, nbytes
        self.t = torch.full((self.lo + nbytes + CANARY + 16,), FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[self.lo:self.lo + nbytes]
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + self.lo)

    def host(self, n=None):
        h = self.t.cpu().numpy()
        return h[self.lo:self.lo + (self.n if n is None else n)].tobytes()

    def canaries_ok(self):
        h = self.t.cpu().numpy()
        return bool((h[:self.lo] == FILL).all() and (h[self.lo + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.t.cpu().numpy() == FILL).all())


class Rig:
    def __init__(self, torch, gs):
        self.torch, self.gs = torch, gs
        self.outs, self.word_ts, self.wss = [], [], []
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(20240611)

    def stream(self):
        return self.torch.cuda.stream(self.gs.torch_stream)

    def out(self, nbytes, shift=0):
        g = Guarded(self.torch, nbytes, shift)
        self.outs.append(g)
        return g

    def buf(self, nbytes, shift=0):
        """An input buffer (not refilled by scrub)."""
        return Guarded(self.torch, nbytes, shift)

    def words(self, n=1):
        t = self.torch.full((max(n, 1),), SENTINEL, dtype=self.torch.int64, device="cuda")
        self.word_ts.append(t)
        return t

    def ws(self, nbytes):
        """A workspace of exactly `nbytes` bytes."""
        assert nbytes > 0
        t = self.torch.empty((nbytes,), dtype=self.torch.uint8, device="cuda")
        assert t.data_ptr() % 256 == 0
        self.wss.append(t)
        return t

    def scrub(self, fill):
        """Outputs to 0xA5, result words to the sentinel, every workspace byte
        to `fill` -- on the capture stream."""
        for g in self.outs:
            g.t.fill_(FILL)
        for t in self.word_ts:
            t.fill_(SENTINEL)
        for w in self.wss:
            if fill == "random":
                w.copy_(self.torch.randint(0, 256, (w.numel(),), dtype=self.torch.uint8, device="cuda",
                                           generator=self.gen))
            else:
                w.fill_(fill)


def drive(rig, label, call, load, check, want=0, nvar=3, after_capture=None, variant=0, lib=None):
    """Steps 2-5 of the module docstring for one entry.  load(k) writes replay
    content k in place (stream-ordered), check(k) compares everything after a
    synchronise.  `variant` is set for the warm-up and the capture only.
    Returns the captured graph, instantiated; the caller destroys it."""
    torch, gs = rig.torch, rig.gs
    torch.cuda.synchronize()
    if variant:
        assert lib.bshuf_set_variant(variant) == 0
    try:
        with rig.stream():
            load(0)
            rig.scrub(0xFF)
            rc = call()
        gs.synchronize()
        assert rc == want, "%s: the uncaptured call returned %d" % (label, rc)
        check(0)
        g = gs.capture(call, want)
    finally:
        if variant:
            assert lib.bshuf_set_variant(0) == 0
    try:
        print("graph %-44s %3d nodes, linear=%s, kinds=%s" % (label + ("/tickets" if variant else ""), g.nodes,
                                                              g.is_linear_chain(), sorted(set(g.names()))))
        assert g.nodes >= 1, label
        assert H.MEM_ALLOC not in g.types and H.MEM_FREE not in g.types, (label, g.names())
        assert set(g.types) <= {H.KERNEL, H.MEMCPY, H.MEMSET}, (label, g.names())
        assert g.is_linear_chain(), (label, g.nodes, g.edges)
        g.instantiate()
        if after_capture:
            after_capture()
        order = [k % nvar for k in (1, 2, 0)]
        for k, fill in zip(order, WS_FILLS):
            with rig.stream():
                load(k)
                rig.scrub(fill)
            g.launch()
            gs.synchronize()
            check(k)
        # back to back: nothing but the stream orders the second replay behind
        # the first and behind the copy between them
        with rig.stream():
            load(2 % nvar)
            rig.scrub(0xFF)
        g.launch()
        with rig.stream():
            load(1 % nvar)
        g.launch()
        gs.synchronize()
        check(1 % nvar)
    except BaseException:
        gs.hip.hipStreamSynchronize(gs.handle)
        g.destroy()
        raise
    return g


def run(rig, *a, **kw):
    g = drive(rig, *a, **kw)
    rig.gs.synchronize()
    g.destroy()


def put(dst, src):
    """src's bytes to the front of dst (what lies behind stays as it was)."""
    if src.numel():
        dst[:src.numel()].copy_(src)


# ---- 1. the transposes -----------------------------------------------------------
@pytest.mark.parametrize("fwd", [True, False], ids=["shuffle", "unshuffle"])
@pytest.mark.parametrize("shape,variant", [("S1", 0), ("S1", TICKETS), ("S2", 0)], ids=["S1", "S1-tickets", "S2"])
def test_transposes(bs, torch, oracle, gs, shape, fwd, variant):
    sh = SHAPES[shape]
    vs = variants_of(oracle, torch, sh, "abc")
    shuf = [oracle.bitshuffle(C.view_e(v.raw, sh.E), sh.bsz).view(np.uint8).reshape(-1) for v in vs]
    src = [torch.from_numpy(s.copy()).cuda() for s in shuf] if not fwd else [v.d_raw for v in vs]
    want = [v.raw for v in vs] if not fwd else shuf
    rig = Rig(torch, gs)
    inp, out = rig.buf(sh.nbytes, sh.shift), rig.out(sh.nbytes, sh.shift)
    fn = bs.lib.bshuf_bitshuffle_dev if fwd else bs.lib.bshuf_bitunshuffle_dev

    def call():
        return fn(inp.ptr, out.ptr, sh.n, sh.E, sh.block, gs.handle)

    def check(k):
        assert out.host() == want[k].tobytes(), (shape, fwd, k)
        assert out.canaries_ok() and inp.canaries_ok()

    run(rig, "bit%sshuffle_dev %s" % ("" if fwd else "un", shape), call, lambda k: put(inp.view, src[k]), check,
        want=sh.nbytes, variant=variant, lib=bs.lib)


# ---- 2. the encoders ---------------------------------------------------------------
def encode_case(bs, torch, oracle, gs, sh, fast, variant):
    lib = bs.lib
    vs = variants_of(oracle, torch, sh, "abc", fast)
    bound = int(lib.bshuf_compress_lz4_bound(sh.n, sh.E, sh.block))
    rig = Rig(torch, gs)
    inp, out = rig.buf(sh.nbytes, sh.shift), rig.out(bound, sh.shift)
    need = int(lib.bshuf_compress_lz4_dev_workspace(sh.n, sh.E, sh.block))
    assert int(lib.bshuf_lz4_dev_nblocks(sh.n, sh.E, sh.block)) == sh.nb
    ws, res, offs = rig.ws(need), rig.words(1), rig.words(sh.nb)
    fn = lib.bshuf_compress_lz4_fast_dev if fast else lib.bshuf_compress_lz4_dev

    def call():
        return fn(inp.ptr, out.ptr, sh.n, sh.E, sh.block, vp(ws), need, vp(res), vp(offs), gs.handle)

    def check(k):
        v = vs[k]
        assert int(res.item()) == v.stream.size, (sh.name, k)
        got = out.host(v.stream.size)
        assert got == v.stream.tobytes(), (sh.name, k)
        assert offs.cpu().tolist()[:sh.nb] == v.offs, (sh.name, k)
        assert out.canaries_ok() and inp.canaries_ok()
        assert inp.host() == v.raw.tobytes()
        if fast:
            back = oracle.decompress_lz4(np.frombuffer(got, dtype=np.uint8), (sh.n,), C.view_e(v.raw, sh.E).dtype,
                                         sh.bsz)
            assert back.tobytes() == v.raw.tobytes()

    run(rig, "compress_lz4_%sdev %s" % ("fast_" if fast else "", sh.name), call, lambda k: put(inp.view, vs[k].d_raw),
        check, variant=variant, lib=lib)


@pytest.mark.parametrize("shape,variant", [("S1", 0), ("S1", TICKETS), ("S2", 0), ("S3", 0), ("S4", 0), ("S5", 0),
                                           ("S6", TICKETS)],
                         ids=["S1", "S1-tickets", "S2", "S3", "S4", "S5", "S6-tickets"])
def test_compress_exact(bs, torch, oracle, gs, shape, variant):
    """S5 is the pipelined encode's size: captured, it must be one chain on the
    caller's stream (pipe_ctx() refuses a capturing stream)."""
    encode_case(bs, torch, oracle, gs, SHAPES[shape], False, variant)


@pytest.mark.parametrize("shape,variant", [("S1", 0), ("S1", TICKETS), ("S3", 0)], ids=["S1", "S1-tickets", "S3"])
def test_compress_fast(bs, torch, oracle, gs, shape, variant):
    """Against the numpy model of fast parse v1, and decoded back."""
    encode_case(bs, torch, oracle, gs, SHAPES[shape], True, variant)


# ---- 3. the decoder ----------------------------------------------------------------
DECODE_HOWS = ("index", "rebuild", "rebuild-dlen")


@pytest.mark.parametrize("how", DECODE_HOWS)
@pytest.mark.parametrize("shape,variant", [("S1", 0), ("S1", TICKETS), ("S2", 0), ("S3", 0), ("S4", 0),
                                           ("S6", TICKETS)],
                         ids=["S1", "S1-tickets", "S2", "S3", "S4", "S6-tickets"])
def test_decompress(bs, torch, oracle, gs, shape, variant, how):
    """index: the encoder's offsets, three stream lengths in a buffer of
    compress_lz4_bound bytes whose size is the in_nbytes of the call.
    rebuild: offsets NULL, in_nbytes exact, equally long streams.
    rebuild-dlen: offsets NULL, three lengths, the length word on the device."""
    lib, sh = bs.lib, SHAPES[shape]
    vs = variants_of(oracle, torch, sh, "rot" if how == "rebuild" else "abc")
    bound = int(lib.bshuf_compress_lz4_bound(sh.n, sh.E, sh.block))
    cap = vs[0].stream.size if how == "rebuild" else bound
    rig = Rig(torch, gs)
    inp, out = rig.buf(cap, sh.shift), rig.out(sh.nbytes, sh.shift)
    need = int(lib.bshuf_decompress_lz4_dev_workspace(cap, sh.n, sh.E, sh.block))
    ws, res = rig.ws(need), rig.words(1)
    index = torch.zeros(max(sh.nb, 1), dtype=torch.int64, device="cuda")
    dlen = torch.zeros(1, dtype=torch.int64, device="cuda")
    offp = vp(index) if how == "index" else None

    def call():
        if how == "rebuild-dlen":
            return lib.bshuf_decompress_lz4_dev_dlen(inp.ptr, vp(dlen), cap, out.ptr, sh.n, sh.E, sh.block, vp(ws),
                                                     need, vp(res), None, gs.handle)
        return lib.bshuf_decompress_lz4_dev(inp.ptr, cap, out.ptr, sh.n, sh.E, sh.block, vp(ws), need, vp(res), offp,
                                            gs.handle)

    def load(k):
        put(inp.view, vs[k].d_stream)
        index.copy_(vs[k].d_offs)
        dlen.copy_(vs[k].d_len)

    def check(k):
        assert int(res.item()) == vs[k].stream.size, (shape, how, k)
        assert out.host() == vs[k].raw.tobytes(), (shape, how, k)
        assert out.canaries_ok() and inp.canaries_ok()

    run(rig, "decompress_lz4_dev%s %s %s" % ("_dlen" if how == "rebuild-dlen" else "", shape, how), call, load, check,
        variant=variant, lib=lib)


# ---- 4. compress -> decompress_dlen in one graph ---------------------------------------
@pytest.mark.parametrize("shape,variant", [("S1", 0), ("S1", TICKETS), ("S2", 0)], ids=["S1", "S1-tickets", "S2"])
def test_chain_in_one_graph(bs, torch, oracle, gs, shape, variant):
    """The decoder reads the encoder's result word at every replay.  Then the
    decode alone, captured separately, with its length word preset to -91:
    -91 comes back and nothing is written; then good runs of both graphs."""
    lib, sh = bs.lib, SHAPES[shape]
    vs = variants_of(oracle, torch, sh, "abc")
    bound = int(lib.bshuf_compress_lz4_bound(sh.n, sh.E, sh.block))
    rig = Rig(torch, gs)
    inp, comp, back = rig.buf(sh.nbytes, sh.shift), rig.out(bound), rig.out(sh.nbytes, sh.shift)
    ewn = int(lib.bshuf_compress_lz4_dev_workspace(sh.n, sh.E, sh.block))
    dwn = int(lib.bshuf_decompress_lz4_dev_workspace(bound, sh.n, sh.E, sh.block))
    ews, dws, eres, dres = rig.ws(ewn), rig.ws(dwn), rig.words(1), rig.words(1)

    def decode(lenword, res):
        return lib.bshuf_decompress_lz4_dev_dlen(comp.ptr, vp(lenword), bound, back.ptr, sh.n, sh.E, sh.block,
                                                 vp(dws), dwn, vp(res), None, gs.handle)

    def call():
        rc = lib.bshuf_compress_lz4_dev(inp.ptr, comp.ptr, sh.n, sh.E, sh.block, vp(ews), ewn, vp(eres), None,
                                        gs.handle)
        return rc or decode(eres, dres)

    def check(k):
        n = vs[k].stream.size
        assert int(eres.item()) == n and int(dres.item()) == n, (shape, k)
        assert comp.host(n) == vs[k].stream.tobytes()
        assert back.host() == vs[k].raw.tobytes(), (shape, k)
        assert comp.canaries_ok() and back.canaries_ok()

    g = drive(rig, "compress_lz4_dev -> decompress_lz4_dev_dlen %s" % shape, call, lambda k: put(inp.view, vs[k].d_raw),
              check, variant=variant, lib=lib)
    g2 = None
    try:
        # comp holds content 1's stream (the last replay); the decode alone, with a
        # length word of its own
        lenword = torch.full((1,), -91, dtype=torch.int64, device="cuda")
        alone = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g2 = gs.capture(lambda: decode(lenword, alone))
        assert g2.is_linear_chain() and set(g2.types) <= {H.KERNEL, H.MEMCPY, H.MEMSET}, g2.names()
        g2.instantiate()
        with rig.stream():
            back.t.fill_(FILL)
            rig.wss[1].fill_(0xFF)
        g2.launch()
        gs.synchronize()
        assert int(alone.item()) == -91
        assert back.untouched()
        with rig.stream():
            lenword.fill_(vs[1].stream.size)
            alone.fill_(SENTINEL)
        g2.launch()
        gs.synchronize()
        assert int(alone.item()) == vs[1].stream.size
        assert back.host() == vs[1].raw.tobytes() and back.canaries_ok()
        # and the chain again: the error did not stick anywhere
        with rig.stream():
            put(inp.view, vs[0].d_raw)
            rig.scrub("random")
        g.launch()
        gs.synchronize()
        check(0)
    finally:
        gs.hip.hipStreamSynchronize(gs.handle)
        if g2 is not None:
            g2.destroy()
        g.destroy()


# ---- 5. the index alone ----------------------------------------------------------------
def serial_index_status(buf, Cb, nb):
    """What the rebuild reports for the framed region buf[:Cb], by a serial
    walk: the offsets of the headers it can place (-1, the all-ones sentinel,
    for the others) and the status word of csrc/lz4_decode.hip -- 1 for a
    broken link (k_idx_walk: a header that is cut, zero, or whose record runs
    past Cb), 2 for a header count other than nb (k_idx_check), the larger of
    the two when both apply, 0 when the records tile the region."""
    offs, p, broken = [], 0, False
    while p < Cb:
        n = int.from_bytes(buf[p:p + 4].tobytes(), "big") if p + 4 <= Cb else 0
        if n == 0 or p + 4 + n > Cb:
            broken = True
            break
        offs.append(p)
        p += 4 + n
    status = 2 if len(offs) != nb else (1 if broken else 0)
    return (offs + [-1] * nb)[:nb], status


@VARIANTS
@pytest.mark.parametrize("cut", [0, 1], ids=["whole", "cut-by-one-byte"])
def test_block_index(bs, torch, oracle, gs, variant, cut):
    lib, sh = bs.lib, S1
    vs = variants_of(oracle, torch, sh, "rot")
    nbytes = vs[0].stream.size - cut
    rig = Rig(torch, gs)
    inp = rig.buf(nbytes)
    need = int(lib.bshuf_decompress_lz4_dev_workspace(nbytes, sh.n, sh.E, sh.block))
    ws, offs, status = rig.ws(need), rig.words(sh.nb), rig.words(1)

    def call():
        return lib.bshuf_lz4_block_index_dev(inp.ptr, nbytes, sh.n, sh.E, sh.block, vp(ws), need, vp(offs), vp(status),
                                             gs.handle)

    tail = (sh.n % 8) * sh.E
    want = [serial_index_status(v.stream[:nbytes], nbytes - tail, sh.nb) for v in vs]
    if cut:     # the last record no longer fits: its block is not placed, one header is missing
        assert all(w == (v.offs[:-1] + [-1], 2) for w, v in zip(want, vs))
    else:
        assert all(w == (v.offs, 0) for w, v in zip(want, vs))

    def check(k):
        assert int(status.item()) == want[k][1], k
        assert offs.cpu().tolist() == want[k][0], k
        assert inp.canaries_ok()

    run(rig, "lz4_block_index_dev S1 %s" % ("cut" if cut else "whole"), call,
        lambda k: inp.view.copy_(vs[k].d_stream[:nbytes]), check, variant=variant, lib=lib)


# ---- 6. the batch entries ----------------------------------------------------------------
BATCH_SIZES = [4096 * 5 + 11, 777, 4096 * 2, 0, 9000]    # int16 elements
BATCH_BLOCK, BATCH_E = 4096, 2
RING_AND_MORE = 20      # uncaptured batch calls after the capture: more than the ring of 16 table buffers


class Batch:
    """The five streams' replay contents: per stream three Vars."""

    def __init__(self, oracle, torch, lib, family, sizes=BATCH_SIZES, E=BATCH_E, block=BATCH_BLOCK):
        self.sizes, self.E, self.block = sizes, E, block
        self.nbs = [int(lib.bshuf_lz4_dev_nblocks(n, E, block)) for n in sizes]
        self.bounds = [int(lib.bshuf_compress_lz4_bound(n, E, block)) for n in sizes]
        self.vars = []
        for i, (n, nb) in enumerate(zip(sizes, self.nbs)):
            raws = (abc_contents(oracle, n * E, seed=i) if family == "abc"
                    else rot_contents(oracle, n * E, E, block, seed=i))
            self.vars.append([Var(oracle, torch, r, E, block, nb) for r in raws])
            lens = [v.stream.size for v in self.vars[-1]]
            assert n == 0 or len(set(lens)) == (3 if family == "abc" else 1), (i, lens)
            assert n == 0 or all_differ(self.vars[-1]), i


_BATCHES = {}


def batch_of(oracle, torch, lib, family):
    if family not in _BATCHES:
        _BATCHES[family] = Batch(oracle, torch, lib, family)
    return _BATCHES[family]


def arrays(ptrs=None, sizes=None):
    from bitshuffle_amd.api import _ptr_array, _size_array
    return _ptr_array(ptrs) if ptrs is not None else _size_array(sizes)


def test_batch_compress(bs, torch, oracle, gs):
    lib = bs.lib
    B = batch_of(oracle, torch, lib, "abc")
    count = len(B.sizes)

    def make():
        rig = Rig(torch, gs)
        ins = [rig.buf(n * B.E) for n in B.sizes]
        outs = [rig.out(b) for b in B.bounds]
        psz, k1 = arrays(sizes=B.sizes)
        need = int(lib.bshuf_compress_lz4_batch_dev_workspace(psz, count, B.E, B.block))
        ws, res, offs = rig.ws(need), rig.words(count), rig.words(sum(B.nbs))
        pin, k2 = arrays(ptrs=[g.ptr.value for g in ins])
        pout, k3 = arrays(ptrs=[g.ptr.value for g in outs])

        def call():
            return lib.bshuf_compress_lz4_batch_dev(pin, pout, psz, count, B.E, B.block, vp(ws), need, vp(res),
                                                    vp(offs), gs.handle)
        return rig, ins, outs, res, offs, call, (k1, k2, k3)

    rig, ins, outs, res, offs, call, keep = make()
    other = make()

    def load(k, ins=ins):
        for g, v in zip(ins, B.vars):
            put(g.view, v[k].d_raw)

    def check(k):
        assert res.cpu().tolist() == [v[k].stream.size for v in B.vars], k
        assert offs.cpu().tolist() == [o for v in B.vars for o in v[k].offs], k
        for g, v in zip(outs, B.vars):
            assert g.host(v[k].stream.size) == v[k].stream.tobytes(), k
            assert g.canaries_ok()

    def crowd():
        with rig.stream():
            load(2, other[1])
            for _ in range(RING_AND_MORE):
                assert other[5]() == 0
        gs.synchronize()

    run(rig, "compress_lz4_batch_dev", call, load, check, after_capture=crowd)


@pytest.mark.parametrize("dlen", [False, True], ids=["host-lengths", "device-lengths"])
def test_batch_decompress(bs, torch, oracle, gs, dlen):
    """Host lengths: equally long streams (the index is rebuilt from exact
    lengths).  Device lengths: three lengths per stream, capacities of
    compress_lz4_bound bytes.  After the capture 20 uncaptured batch calls go
    through the thread's ring of 16 table buffers; then the replays; then a
    replay with stream 0's first header zeroed, and one with it restored."""
    lib = bs.lib
    B = batch_of(oracle, torch, lib, "abc" if dlen else "rot")
    count = len(B.sizes)
    caps = B.bounds if dlen else [v[0].stream.size for v in B.vars]

    def make():
        rig = Rig(torch, gs)
        ins = [rig.buf(c) for c in caps]
        outs = [rig.out(n * B.E) for n in B.sizes]
        psz, k1 = arrays(sizes=B.sizes)
        pcap, k2 = arrays(sizes=caps)
        need = int(lib.bshuf_decompress_lz4_batch_dev_workspace(pcap, psz, count, B.E, B.block))
        ws, res = rig.ws(need), rig.words(count)
        lens = torch.zeros(count, dtype=torch.int64, device="cuda")
        pin, k3 = arrays(ptrs=[g.ptr.value for g in ins])
        pout, k4 = arrays(ptrs=[g.ptr.value for g in outs])

        def call():
            if dlen:
                return lib.bshuf_decompress_lz4_batch_dev_dlen(pin, vp(lens), pcap, pout, psz, count, B.E, B.block,
                                                               vp(ws), need, vp(res), gs.handle)
            return lib.bshuf_decompress_lz4_batch_dev(pin, pcap, pout, psz, count, B.E, B.block, vp(ws), need, vp(res),
                                                      gs.handle)
        return rig, ins, outs, res, lens, call, (k1, k2, k3, k4)

    rig, ins, outs, res, lens, call, keep = make()
    other = make()
    d_lens = [torch.tensor([v[k].stream.size for v in B.vars], dtype=torch.int64, device="cuda") for k in range(3)]

    def load(k, ins=ins, lens=lens):
        for g, v in zip(ins, B.vars):
            put(g.view, v[k].d_stream)
        lens.copy_(d_lens[k])

    def check(k, skip=()):
        got = res.cpu().tolist()
        for i, (g, v) in enumerate(zip(outs, B.vars)):
            if i in skip:
                continue
            assert got[i] == v[k].stream.size, (k, i, got)
            assert g.host() == v[k].raw.tobytes(), (k, i)
            assert g.canaries_ok()

    def crowd():
        with rig.stream():
            load(2, other[1], other[4])
            for _ in range(RING_AND_MORE):
                assert other[5]() == 0
        gs.synchronize()

    g = drive(rig, "decompress_lz4_batch_dev%s" % ("_dlen" if dlen else ""), call, load, check, after_capture=crowd)
    try:
        bad = B.vars[0][2].stream.copy()
        bad[:4] = 0
        with pytest.raises(RuntimeError) as orc:
            oracle.decompress_lz4(bad, (B.sizes[0],), np.int16, B.block)
        code = int(orc.value.args[1])
        assert code < 0
        with rig.stream():
            load(2)
            rig.scrub(0x00)
            ins[0].view[:4].zero_()
        g.launch()
        gs.synchronize()
        assert int(res[0].item()) == code, (int(res[0].item()), code)
        assert outs[0].canaries_ok()
        check(2, skip=(0,))
        with rig.stream():
            load(2)
            rig.scrub("random")
        g.launch()
        gs.synchronize()
        check(2)
    finally:
        gs.hip.hipStreamSynchronize(gs.handle)
        g.destroy()


# ---- 7. the batch encode's per-stream route with a caller workspace -----------------------
# blocks above the LDS encoder's size; blocks that need the byU32 table with
# partial blocks that need the byU16 one (both table types in one batch)
WIDE_BLOCK = C.above(M.U16_TABLE_LIMIT - 1, 4) // 4
PER_STREAM = {"large-blocks": (S4_BLOCK, [S4.n, S4_BLOCK + 16 * 8 + 5]),
              "both-table-types": (WIDE_BLOCK, [2 * WIDE_BLOCK + 1000 + 5, WIDE_BLOCK + 520 + 3])}


@pytest.mark.parametrize("route", list(PER_STREAM))
def test_batch_compress_per_stream_route_in_the_callers_workspace(bs, torch, oracle, gs, route):
    """Batches that are encoded one stream at a time: with a caller workspace
    of bshuf_compress_lz4_batch_dev_workspace() bytes that route too allocates
    nothing: no MemAlloc / MemFree node."""
    lib = bs.lib
    block, sizes = PER_STREAM[route]
    assert M.encode_batch(4, block, sizes, [0] * len(sizes))[0] == "per-stream"
    B = Batch(oracle, torch, lib, "abc", sizes=sizes, E=4, block=block)
    count = len(sizes)
    rig = Rig(torch, gs)
    ins = [rig.buf(n * B.E) for n in sizes]
    outs = [rig.out(b) for b in B.bounds]
    psz, k1 = arrays(sizes=sizes)
    need = int(lib.bshuf_compress_lz4_batch_dev_workspace(psz, count, B.E, B.block))
    assert need >= max(int(lib.bshuf_compress_lz4_dev_workspace(n, B.E, B.block)) for n in sizes)
    ws, res, offs = rig.ws(need), rig.words(count), rig.words(sum(B.nbs))
    pin, k2 = arrays(ptrs=[g.ptr.value for g in ins])
    pout, k3 = arrays(ptrs=[g.ptr.value for g in outs])

    def call():
        return lib.bshuf_compress_lz4_batch_dev(pin, pout, psz, count, B.E, B.block, vp(ws), need, vp(res), vp(offs),
                                                gs.handle)

    def load(k):
        for g, v in zip(ins, B.vars):
            put(g.view, v[k].d_raw)

    def check(k):
        assert res.cpu().tolist() == [v[k].stream.size for v in B.vars], k
        assert offs.cpu().tolist() == [o for v in B.vars for o in v[k].offs], k
        for g, v in zip(outs, B.vars):
            assert g.host(v[k].stream.size) == v[k].stream.tobytes(), k
            assert g.canaries_ok()

    run(rig, "compress_lz4_batch_dev %s" % route, call, load, check)


def test_batch_decompress_large_blocks_in_the_callers_workspace(bs, torch, oracle, gs):
    """The decoder's per-stream route (blocks above the LDS decoder's size),
    the same way."""
    lib = bs.lib
    sizes = [S4.n, S4_BLOCK + 16 * 8 + 5]
    B = Batch(oracle, torch, lib, "rot", sizes=sizes, E=4, block=S4_BLOCK)
    count = len(sizes)
    caps = [v[0].stream.size for v in B.vars]
    rig = Rig(torch, gs)
    ins = [rig.buf(c) for c in caps]
    outs = [rig.out(n * B.E) for n in sizes]
    psz, k1 = arrays(sizes=sizes)
    pcap, k2 = arrays(sizes=caps)
    need = int(lib.bshuf_decompress_lz4_batch_dev_workspace(pcap, psz, count, B.E, B.block))
    assert need >= max(int(lib.bshuf_decompress_lz4_dev_workspace(c, n, B.E, B.block)) for c, n in zip(caps, sizes))
    ws, res = rig.ws(need), rig.words(count)
    pin, k3 = arrays(ptrs=[g.ptr.value for g in ins])
    pout, k4 = arrays(ptrs=[g.ptr.value for g in outs])

    def call():
        return lib.bshuf_decompress_lz4_batch_dev(pin, pcap, pout, psz, count, B.E, B.block, vp(ws), need, vp(res),
                                                  gs.handle)

    def load(k):
        for g, v in zip(ins, B.vars):
            put(g.view, v[k].d_stream)

    def check(k):
        assert res.cpu().tolist() == caps, k
        for g, v in zip(outs, B.vars):
            assert g.host() == v[k].raw.tobytes(), k
            assert g.canaries_ok()

    run(rig, "decompress_lz4_batch_dev large blocks", call, load, check)


# ---- 8. ranges ---------------------------------------------------------------------------
RANGES = [(0, 1), (4095, 3), (S1.n - 5, 5), (8192, 4096), (100, 0)]


@VARIANTS
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("with_index", [True, False], ids=["index", "rebuild"])
def test_ranges(bs, torch, oracle, gs, variant, with_index, shift):
    """The ranges stay, the stream's contents change.  With the index: three
    stream lengths in a buffer of compress_lz4_bound bytes, which is the call's
    in_nbytes.  Without: equally long streams, in_nbytes exact."""
    lib, sh = bs.lib, S1
    vs = variants_of(oracle, torch, sh, "abc" if with_index else "rot")
    cap = int(lib.bshuf_compress_lz4_bound(sh.n, sh.E, sh.block)) if with_index else vs[0].stream.size
    total = sum(c for _, c in RANGES) * sh.E
    want = [b"".join(v.raw[s * sh.E:(s + c) * sh.E].tobytes() for s, c in RANGES) for v in vs]
    rig = Rig(torch, gs)
    inp, out = rig.buf(cap), rig.out(total, shift)
    pst, k1 = arrays(sizes=[s for s, _ in RANGES])
    pct, k2 = arrays(sizes=[c for _, c in RANGES])
    need = int(lib.bshuf_decompress_lz4_ranges_dev_workspace(cap, sh.n, sh.E, sh.block, pst, pct, len(RANGES)))
    ws, res = rig.ws(need), rig.words(1)
    index = torch.zeros(sh.nb, dtype=torch.int64, device="cuda")

    def call():
        return lib.bshuf_decompress_lz4_ranges_dev(inp.ptr, cap, sh.n, sh.E, sh.block, pst, pct, len(RANGES), out.ptr,
                                                   vp(ws), need, vp(res), vp(index) if with_index else None, gs.handle)

    def load(k):
        put(inp.view, vs[k].d_stream)
        index.copy_(vs[k].d_offs)

    def check(k):
        assert int(res.item()) == total, k
        assert out.host() == want[k], k
        assert out.canaries_ok() and inp.canaries_ok()

    run(rig, "decompress_lz4_ranges_dev S1 %s %s" % ("index" if with_index else "rebuild", "odd" if shift else "al"),
        call, load, check, variant=variant, lib=lib)


# ---- 9. the stream set -------------------------------------------------------------------
@VARIANTS
def test_stream_set_build(bs, torch, oracle, gs, variant):
    """A captured build over three S1-sized streams without supplied indexes;
    the streams are overwritten in place with other encodings of their length
    and the build replayed; after each replay an uncaptured window decode over
    the set gives four windows per stream exactly."""
    lib, sh = bs.lib, S1
    vs = variants_of(oracle, torch, sh, "rot")
    count, window = 3, 1500
    nbytes = vs[0].stream.size
    rig = Rig(torch, gs)
    ins = [rig.buf(nbytes) for _ in range(count)]
    psz, k1 = arrays(sizes=[sh.n] * count)
    pnb, k2 = arrays(sizes=[nbytes] * count)
    pin, k3 = arrays(ptrs=[g.ptr.value for g in ins])
    set_bytes = int(lib.bshuf_lz4_stream_set_dev_bytes(psz, count, sh.E, sh.block))
    need = int(lib.bshuf_lz4_stream_set_dev_workspace(pnb, psz, count, sh.E, sh.block))
    assert set_bytes > 0 and need > 0
    d_set = torch.zeros(set_bytes, dtype=torch.uint8, device="cuda")
    assert d_set.data_ptr() % 256 == 0
    ws, status = rig.ws(need), rig.words(count)
    # the windows: block-aligned, straddling a boundary, partial block + tail, mid-block
    st = [0, 4095, sh.n - window, 8192 + 5]
    ids = torch.tensor([s for s in range(count) for _ in st], dtype=torch.int64, device="cuda")
    starts = torch.tensor(st * count, dtype=torch.int64, device="cuda")
    K = count * len(st)
    wout = Guarded(torch, K * window * sh.E)
    wneed = int(lib.bshuf_decompress_lz4_windows_set_dev_workspace(sh.n, sh.E, sh.block, K, window))
    wws = torch.empty(wneed, dtype=torch.uint8, device="cuda")
    wres = torch.zeros(1, dtype=torch.int64, device="cuda")
    wstat = torch.zeros(K, dtype=torch.int64, device="cuda")

    def call():
        return lib.bshuf_lz4_stream_set_dev(pin, pnb, psz, count, sh.E, sh.block, None, vp(d_set), set_bytes, vp(ws),
                                            need, vp(status), gs.handle)

    def load(k):
        for j, g in enumerate(ins):
            g.view.copy_(vs[(k + j) % 3].d_stream)

    def check(k):
        assert status.cpu().tolist() == [0] * count, k
        with rig.stream():
            wout.t.fill_(FILL)
            wres.fill_(SENTINEL)
            rc = lib.bshuf_decompress_lz4_windows_set_dev(vp(d_set), count, sh.n, sh.E, sh.block, vp(ids), vp(starts),
                                                          K, window, wout.ptr, vp(wws), wneed, vp(wres), vp(wstat),
                                                          gs.handle)
        gs.synchronize()
        assert rc == 0 and int(wres.item()) == K * window * sh.E, k
        assert wstat.cpu().tolist() == [window * sh.E] * K
        want = b"".join(vs[(k + j) % 3].raw[s * sh.E:(s + window) * sh.E].tobytes() for j in range(count) for s in st)
        assert wout.host() == want, k
        assert wout.canaries_ok() and all(g.canaries_ok() for g in ins)

    run(rig, "lz4_stream_set_dev 3 x S1", call, load, check, variant=variant, lib=lib)

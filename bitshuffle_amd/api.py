"""numpy / torch front end over the C-ABI.

Host functions mirror bitshuffle/ext.pyx of the reference one for one
(argument names, C-contiguity check, `out=` reuse, RuntimeError("Failed.
Error code %d.", code) on negative returns, and decompress_lz4's check that
the whole input buffer was consumed, ext.pyx:501-504).  Unlike the Cython
wrapper, sizes are 64-bit, so arrays beyond 2**31 elements work.

Device functions take torch tensors that live on a HIP device and enqueue on
the current torch stream (or `stream=`); nothing is copied to the host except
the compressed length when `sync=True`.
"""
import ctypes

import numpy as np

from ._lib import CVT_DST, CVT_SRC, BshufError, Cvt, lib


def _fail(code, what="Failed. Error code %d."):
    raise BshufError(what % code, int(code))


def _check(code):
    if code < 0:
        _fail(code)
    return code


def _make_array(shape, dtype, out=None):
    # bitshuffle/ext.pyx:124-133
    if out is None:
        return np.empty(shape, dtype=dtype)
    size = int(np.prod(shape))
    base = out if out.base is None else out.base
    return base.ravel().view(dtype)[:size].reshape(shape)


def _setup_arr(arr, out=None):
    # bitshuffle/ext.pyx:136-145
    if not arr.flags["C_CONTIGUOUS"]:
        raise ValueError("Input array must be C-contiguous.")
    return _make_array(tuple(arr.shape), arr.dtype, out), arr.size, arr.dtype.itemsize


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def default_block_size(elem_size):
    return int(lib.bshuf_default_block_size(elem_size))


def compress_lz4_bound(size, elem_size, block_size=0):
    return int(lib.bshuf_compress_lz4_bound(size, elem_size, block_size))


# ---------------------------------------------------------------- host API
def bitshuffle(arr, block_size=0, out=None):
    """Bitshuffle an array (reference bitshuffle/ext.pyx:311-353)."""
    out, size, itemsize = _setup_arr(arr, out)
    _check(lib.bshuf_bitshuffle(_ptr(arr), _ptr(out), size, itemsize, block_size))
    return out


def bitunshuffle(arr, block_size=0, out=None):
    """Undo bitshuffle (reference bitshuffle/ext.pyx:356-398)."""
    out, size, itemsize = _setup_arr(arr, out)
    _check(lib.bshuf_bitunshuffle(_ptr(arr), _ptr(out), size, itemsize, block_size))
    return out


# The parse rule mode="fast" follows ("fast parse v1").
FAST_PARSE_VERSION = int(lib.bshuf_lz4_fast_version())


def _mode(mode, exact, fast):
    """The entry point of an encode mode: "exact" (the reference encoder's
    bytes) or "fast" (same format, fixed-offset parse, other bytes)."""
    if mode == "exact":
        return exact
    if mode == "fast":
        return fast
    raise ValueError("mode must be 'exact' or 'fast', not %r" % (mode,))


def compress_lz4(arr, block_size=0, out=None, mode="exact"):
    """Bitshuffle then LZ4-compress; returns the framed uint8 stream
    (reference bitshuffle/ext.pyx:401-447).  mode="fast": the fast parse
    (any bitshuffle/LZ4 reader decodes it; not the reference encoder's bytes)."""
    fn = _mode(mode, lib.bshuf_compress_lz4, lib.bshuf_compress_lz4_fast)
    if not arr.flags["C_CONTIGUOUS"]:
        raise ValueError("Input array must be C-contiguous.")
    size, itemsize = arr.size, arr.dtype.itemsize
    bound = compress_lz4_bound(size, itemsize, block_size)
    if bound > (1 << 62):  # the (size_t)-81 quirk of an invalid block size
        _fail(-81)
    out = _make_array((max(bound, 1),), np.uint8, out)
    count = _check(fn(_ptr(arr), _ptr(out), size, itemsize, block_size))
    return out[:count]


def decompress_lz4(arr, shape, dtype, block_size=0, out=None):
    """LZ4-decompress then bitunshuffle (reference bitshuffle/ext.pyx:452-505)."""
    if not arr.flags["C_CONTIGUOUS"]:
        raise ValueError("Input array must be C-contiguous.")
    dtype = np.dtype(dtype)
    size = int(np.prod(shape))
    out = _make_array(tuple(shape), dtype, out)
    count = _check(lib.bshuf_decompress_lz4(_ptr(arr), _ptr(out), size, dtype.itemsize,
                                            block_size))
    if count != arr.size:
        msg = "Decompressed different number of bytes than input buffer size."
        msg += "Input buffer %d, decompressed %d." % (arr.size, count)
        raise BshufError(msg, count)
    return out


# -------------------------------------------------------------- device API
def _torch():
    import torch
    return torch


def _stream(stream):
    torch = _torch()
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


def _dptr(t):
    if not t.is_cuda:
        raise ValueError("device functions need a HIP (torch 'cuda') tensor")
    if not t.is_contiguous():
        raise ValueError("Input array must be C-contiguous.")
    return ctypes.c_void_p(t.data_ptr())


def bitshuffle_dev(t, block_size=0, out=None, stream=None):
    out = _torch().empty_like(t) if out is None else out
    _check(lib.bshuf_bitshuffle_dev(_dptr(t), _dptr(out), t.numel(), t.element_size(),
                                    block_size, _stream(stream)))
    return out


def bitunshuffle_dev(t, block_size=0, out=None, stream=None):
    out = _torch().empty_like(t) if out is None else out
    _check(lib.bshuf_bitunshuffle_dev(_dptr(t), _dptr(out), t.numel(), t.element_size(),
                                      block_size, _stream(stream)))
    return out


def compress_lz4_workspace(numel, elem_size, block_size=0, device=None):
    torch = _torch()
    n = int(lib.bshuf_compress_lz4_dev_workspace(numel, elem_size, block_size))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def decompress_lz4_workspace(in_nbytes, numel, elem_size, block_size=0, device=None):
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_dev_workspace(in_nbytes, numel, elem_size, block_size))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def _elems(t, elem_size):
    """(element count, element size) of tensor t; elem_size overrides the
    dtype's, for element sizes torch has no dtype for (t is then raw bytes)."""
    if elem_size is None:
        return t.numel(), t.element_size()
    nbytes = t.numel() * t.element_size()
    if elem_size <= 0 or nbytes % elem_size:
        raise ValueError("tensor of %d bytes is not a whole number of %d-byte elements"
                         % (nbytes, elem_size))
    return nbytes // elem_size, int(elem_size)


def compress_lz4_dev(t, block_size=0, out=None, workspace=None, result=None, offsets=None,
                     stream=None, sync=True, elem_size=None, mode="exact"):
    """Device-resident bshuf_compress_lz4.  Returns the framed stream as a uint8
    tensor view (sync=True), or (out, result) where result is a 1-element int64
    device tensor holding the byte count / error (sync=False).  `elem_size`
    overrides the tensor's element size (any E, e.g. a uint8 tensor of
    7-byte records).  mode="fast" selects bshuf_compress_lz4_fast_dev."""
    torch = _torch()
    fn = _mode(mode, lib.bshuf_compress_lz4_dev, lib.bshuf_compress_lz4_fast_dev)
    n, es = _elems(t, elem_size)
    bound = compress_lz4_bound(n, es, block_size)
    if bound > (1 << 62):
        _fail(-81)
    if out is None:
        out = torch.empty(max(bound, 1), dtype=torch.uint8, device=t.device)
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=t.device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    offp = _dptr(offsets) if offsets is not None else None
    _check(fn(_dptr(t), _dptr(out), n, es, block_size, ws, wsb, _dptr(result), offp, _stream(stream)))
    if not sync:
        return out, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    return out[:count]


def decompress_lz4_dev(buf, shape, dtype, block_size=0, out=None, workspace=None, result=None,
                       offsets=None, stream=None, sync=True, elem_size=None, length=None):
    """Device-resident bshuf_decompress_lz4 of the whole uint8 tensor `buf`
    (its length is the exact stream length).  With `elem_size`, `shape` counts
    elem_size-byte elements and the output is a uint8 tensor of their bytes.
    With `length` (a 1-element int64 DEVICE tensor, e.g. compress_lz4_dev's
    `result` with sync=False), the stream length is read on the device
    (bshuf_decompress_lz4_dev_dlen) and `buf` is only its capacity: nothing
    waits on the host between the two calls."""
    torch = _torch()
    size = 1
    for s in shape:
        size *= int(s)
    if out is None:
        if elem_size is None:
            out = torch.empty(tuple(shape), dtype=dtype, device=buf.device)
        else:
            out = torch.empty(size * int(elem_size), dtype=torch.uint8, device=buf.device)
    es = out.element_size() if elem_size is None else int(elem_size)
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=buf.device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    offp = _dptr(offsets) if offsets is not None else None
    if length is None:
        _check(lib.bshuf_decompress_lz4_dev(_dptr(buf), buf.numel(), _dptr(out), size,
                                            es, block_size, ws, wsb, _dptr(result),
                                            offp, _stream(stream)))
    else:
        if length.dtype != torch.int64 or length.numel() < 1 or length.device != buf.device:
            raise ValueError("length must be an int64 tensor on the stream's device")
        _check(lib.bshuf_decompress_lz4_dev_dlen(_dptr(buf), _dptr(length), buf.numel(), _dptr(out),
                                                 size, es, block_size, ws, wsb, _dptr(result),
                                                 offp, _stream(stream)))
    if not sync:
        return out, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    want = buf.numel() if length is None else int(length.reshape(-1)[0].item())
    if count != want:
        raise BshufError("Decompressed different number of bytes than input buffer size."
                         "Input buffer %d, decompressed %d." % (want, count)
                         + ("" if length is None else " (buffer capacity %d)" % buf.numel()), count)
    return out


def _range_arrays(ranges):
    starts, counts = [], []
    for start, count in ranges:
        start, count = int(start), int(count)
        if start < 0 or count < 0:
            raise ValueError("a range is (start, count) with both >= 0, not (%d, %d)" % (start, count))
        starts.append(start)
        counts.append(count)
    ps, keep1 = _size_array(starts)
    pc, keep2 = _size_array(counts)
    return counts, ps, pc, (keep1, keep2)


def decompress_lz4_ranges_workspace(in_nbytes, size, elem_size, ranges, block_size=0, device=None):
    """A workspace for decompress_lz4_ranges_dev of these ranges (or of other
    ranges that touch no more blocks) of a stream of `in_nbytes` bytes."""
    torch = _torch()
    _, ps, pc, keep = _range_arrays(ranges)
    n = int(lib.bshuf_decompress_lz4_ranges_dev_workspace(in_nbytes, size, elem_size, block_size,
                                                          ps, pc, len(ranges)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def decompress_lz4_ranges_dev(buf, size, dtype, ranges, block_size=0, out=None, workspace=None,
                              result=None, offsets=None, stream=None, sync=True, elem_size=None):
    """Random-access decode (bshuf_decompress_lz4_ranges_dev): the element
    ranges `ranges` -- a sequence of (start, count) -- of the framed stream in
    uint8 device tensor `buf`, which encodes `size` elements of `dtype`; only
    the blocks a range touches are decoded.  The ranges' elements land back to
    back in one dense `out`; returns one tensor per range, views of it
    (sync=True), or (out, result) with result a 1-element int64 device tensor
    of the byte count / error code (sync=False).  Ranges may overlap, repeat,
    come in any order and be empty.  `offsets`: the stream's block index
    (compress_lz4_dev's `offsets=` tensor, or block_index_dev's); without it
    the index is rebuilt from the whole stream.  With `elem_size`, size, start
    and count are in elem_size-byte elements and the output is uint8."""
    torch = _torch()
    ranges = list(ranges)
    counts, ps, pc, keep = _range_arrays(ranges)
    total = sum(counts)
    if out is None:
        if elem_size is None:
            out = torch.empty(total, dtype=dtype, device=buf.device)
        else:
            out = torch.empty(total * int(elem_size), dtype=torch.uint8, device=buf.device)
    es = out.element_size() if elem_size is None else int(elem_size)
    if out.numel() * out.element_size() < total * es:
        raise ValueError("out holds %d bytes, the ranges need %d"
                         % (out.numel() * out.element_size(), total * es))
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=buf.device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    offp = _dptr(offsets) if offsets is not None else None
    _check(lib.bshuf_decompress_lz4_ranges_dev(_dptr(buf), buf.numel(), int(size), es, block_size,
                                               ps, pc, len(ranges), _dptr(out), ws, wsb,
                                               _dptr(result), offp, _stream(stream)))
    if not sync:
        return out, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    per = 1 if elem_size is None else es  # out items per element
    flat = out.reshape(-1)
    views, at = [], 0
    for c in counts:
        views.append(flat[at * per:(at + c) * per])
        at += c
    return views


def decompress_lz4_range_dev(buf, size, dtype, start, count, **kw):
    """One range of decompress_lz4_ranges_dev: the tensor of elements
    [start, start + count) (sync=True), or (out, result) (sync=False)."""
    r = decompress_lz4_ranges_dev(buf, size, dtype, [(start, count)], **kw)
    return r if kw.get("sync", True) is False else r[0]


def _dtype_name(dtype):
    torch = _torch()
    return str(dtype).split(".")[-1] if isinstance(dtype, torch.dtype) else np.dtype(dtype).name


def _cvt(dtype, out_dtype, scale, offset, elem_size):
    """The bshuf_cvt of a converting call (out_dtype given), else None: `dtype`
    names the stream's elements, `out_dtype` those of `out`."""
    if out_dtype is None:
        return None
    if elem_size is not None:
        raise ValueError("out_dtype converts elements of `dtype`: it does not go with elem_size=")
    src, dst = CVT_SRC.get(_dtype_name(dtype)), CVT_DST.get(_dtype_name(out_dtype))
    if dst is None:
        raise ValueError("out_dtype must be torch.float32, float16 or bfloat16, not %s" % (out_dtype,))
    if src is None:
        raise ValueError("out_dtype needs a dtype of uint8, int8, uint16, int16, uint32, int32 or float32, not %s"
                         % (dtype,))
    return Cvt(src, dst, float(scale), float(offset))


def _cvt_out(cvt, out, out_dtype):
    """A converting call's `out`: of out_dtype, aligned to it.  Returns the
    stream's element size."""
    if out.dtype != out_dtype:
        raise ValueError("out must be a %s tensor, not %s" % (out_dtype, out.dtype))
    if out.data_ptr() % out.element_size():
        raise ValueError("out must be aligned to its %d-byte elements" % out.element_size())
    return 1 if cvt.src < 2 else 2 if cvt.src < 4 else 4


def _windows_dev(call, device, whose, index, dtype, window, out, workspace, result, status, sync, elem_size,
                 holds=None, cvt=None, out_dtype=None):
    """What the window decodes of one stream and of a set share.  `index`:
    (name, tensor) pairs, the device tensors with one entry per window each;
    `device`: where they must live, called the "`whose` device" in messages.
    `holds`: the element size the set was built with.  call(es, K, window, out,
    ws, ws_bytes, result, status) makes the library call with these arguments
    of its own among the others and returns its code.  cvt, out_dtype: a
    converting call (_cvt): `out` is of out_dtype, sized in its elements."""
    torch = _torch()
    for name, t in index:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                and t.device == device):
            raise ValueError("%s must be a contiguous int64 tensor on the %s device" % (name, whose))
    counts = [t.numel() for _, t in index]
    if len(set(counts)) > 1:
        raise ValueError("%s need one entry per window (%s)" % (" and ".join(name for name, _ in index),
                                                                " and ".join("%d" % n for n in counts)))
    K, window = counts[-1], int(window)
    if window < 0:
        raise ValueError("window must be >= 0, not %d" % window)
    if out is None:
        if cvt is not None:
            out = torch.empty((K, window), dtype=out_dtype, device=device)
        elif elem_size is None:
            out = torch.empty((K, window), dtype=dtype, device=device)
        else:
            out = torch.empty((K, window * int(elem_size)), dtype=torch.uint8, device=device)
    if cvt is not None:
        es = _cvt_out(cvt, out, out_dtype)
    else:
        es = out.element_size() if elem_size is None else int(elem_size)
    if holds is not None and es != holds:
        raise ValueError("the set holds %d-byte elements, not %d-byte ones" % (holds, es))
    per = out.element_size() if cvt is not None else es  # bytes of `out` per element
    if out.numel() * out.element_size() < K * window * per:
        raise ValueError("out holds %d bytes, the windows need %d"
                         % (out.numel() * out.element_size(), K * window * per))
    if status is not None and (status.dtype != torch.int64 or status.numel() < K):
        raise ValueError("status must be an int64 tensor of %d entries" % K)
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    stp = _dptr(status) if status is not None else None
    _check(call(es, K, window, _dptr(out), ws, wsb, _dptr(result), stp))
    if not sync:
        return out, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    return out


def decompress_lz4_windows_workspace(in_nbytes, size, elem_size, nwindows, window, block_size=0,
                                     device=None):
    """A workspace for decompress_lz4_windows_dev of `nwindows` windows of
    `window` elements of a stream of `in_nbytes` bytes: its size depends on
    these numbers only, never on the starts."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_windows_dev_workspace(in_nbytes, size, elem_size, block_size,
                                                           nwindows, window))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def decompress_lz4_windows_dev(buf, size, dtype, starts, window, block_size=0, out=None,
                               workspace=None, result=None, status=None, offsets=None, stream=None,
                               sync=True, elem_size=None, out_dtype=None, scale=1.0, offset=0.0):
    """Window decode (bshuf_decompress_lz4_windows_dev): K = starts.numel()
    windows of `window` elements each of the framed stream in uint8 device
    tensor `buf`, which encodes `size` elements of `dtype`.  `starts` is a
    contiguous int64 DEVICE tensor of element indices, read by the kernels only:
    nothing here copies it to the host, and a call captured into a graph decodes
    whatever starts the tensor holds at each replay.  Returns a (K, window)
    tensor of `dtype` -- with `elem_size` a uint8 tensor (K, window * elem_size)
    -- (sync=True), or (out, result) with result a 1-element int64 device tensor
    of the byte count / error code (sync=False).  `status` (int64 device tensor,
    K entries): per window its byte count, -71 for a start outside [0, size -
    window] (that window's part of `out` is left as it was), or the code of a
    failing block it touches.  `offsets`: the stream's block index; without it
    the index is rebuilt from the whole stream.

    Decode to float (bshuf_decompress_lz4_windows_cvt_dev): with `out_dtype`
    torch.float32, float16 or bfloat16 the (K, window) result is of that dtype
    and every element x lands as out_dtype(fmaf(float32(x), scale, offset)), one
    fp32 fused multiply-add, every rounding to nearest even; `dtype` is then
    uint8, int8, uint16, int16, uint32, int32 or float32 (ValueError otherwise,
    and with elem_size=), a caller's `out` is of out_dtype, and `status` and
    `result` go on counting the stream's bytes."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, window, *ptrs):
        offp = _dptr(offsets) if offsets is not None else None
        args = (_dptr(buf), buf.numel(), int(size), es, block_size, _dptr(starts), K, window, *ptrs, offp,
                _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_windows_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_windows_dev(*args)
    return _windows_dev(call, buf.device, "stream's", [("starts", starts)], dtype, window, out, workspace,
                        result, status, sync, elem_size, cvt=cvt, out_dtype=out_dtype)


class StreamSet:
    """A device-resident table of framed streams that share element and block
    size (bshuf_lz4_stream_set_dev), for decompress_lz4_windows_set_dev.  The
    table points into the streams and the supplied block indexes; `bufs` and
    `offsets` keep them alive.  `status` (int64 device tensor, one entry per
    stream) is 0, or -91 for a stream whose index was rebuilt here and whose
    records do not tile it."""

    def __init__(self, table, bufs, offsets, status, sizes, elem_size, block_size):
        self.table, self.bufs, self.offsets, self.status = table, bufs, offsets, status
        self.sizes = list(sizes)
        self.count = len(self.sizes)
        self.max_size = max(self.sizes) if self.sizes else 0
        self.elem_size, self.block_size = int(elem_size), int(block_size)

    @property
    def device(self):
        return self.table.device


def lz4_stream_set_dev(bufs, sizes, elem_size, block_size=0, offsets=None, workspace=None, stream=None):
    """Build a StreamSet of the framed streams in the uint8 device tensors
    `bufs`; stream s encodes sizes[s] elements of `elem_size` bytes in blocks of
    `block_size`.  `offsets`: None, or per stream its block index (what
    compress_lz4_dev / compress_lz4_batch_dev / block_index_dev wrote) or None;
    a stream without one gets its index rebuilt here, once.  Enqueues only:
    read `.status` for the per-stream outcome of the rebuild."""
    torch = _torch()
    bufs, sizes = list(bufs), [int(n) for n in sizes]
    offsets = [None] * len(bufs) if offsets is None else list(offsets)
    if len(sizes) != len(bufs) or len(offsets) != len(bufs):
        raise ValueError("bufs, sizes and offsets need one entry per stream")
    device = bufs[0].device if bufs else (workspace.device if workspace is not None else torch.device("cuda"))
    for t in bufs + [o for o in offsets if o is not None]:
        _dptr(t)
        if t.device != device:
            raise ValueError("every stream and index of a set lives on one device")
    es, count = int(elem_size), len(bufs)
    psz, keep1 = _size_array(sizes)
    pnb, keep2 = _size_array([b.numel() for b in bufs])
    pin, keep3 = _ptr_array([b.data_ptr() for b in bufs])
    poff, keep4 = _ptr_array([o.data_ptr() if o is not None else 0 for o in offsets])
    nbytes = int(lib.bshuf_lz4_stream_set_dev_bytes(psz, count, es, block_size))
    if nbytes == 0:
        # the build's own refusal, before the device is touched
        _check(lib.bshuf_lz4_stream_set_dev(pin, pnb, psz, count, es, block_size, poff, None, 0, None, 0,
                                            None, _stream(stream)))
        _fail(-71)
    table = torch.empty(nbytes, dtype=torch.uint8, device=device)
    status = torch.zeros(max(count, 1), dtype=torch.int64, device=device)[:count]
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    _check(lib.bshuf_lz4_stream_set_dev(pin, pnb, psz, count, es, block_size, poff, _dptr(table), nbytes,
                                        ws, wsb, ctypes.c_void_p(status.data_ptr()), _stream(stream)))
    return StreamSet(table, bufs, offsets, status, sizes, es, block_size)


def decompress_lz4_windows_set_workspace(sset, nwindows, window, device=None):
    """A workspace for decompress_lz4_windows_set_dev of `nwindows` windows of
    `window` elements over StreamSet `sset`: its size depends on the set's
    largest stream, element and block size and these two numbers only."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_windows_set_dev_workspace(sset.max_size, sset.elem_size,
                                                               sset.block_size, nwindows, window))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or sset.device)


def decompress_lz4_windows_set_dev(sset, dtype, ids, starts, window, out=None, workspace=None, result=None,
                                   status=None, stream=None, sync=True, elem_size=None, out_dtype=None,
                                   scale=1.0, offset=0.0):
    """Window decode over a StreamSet (bshuf_decompress_lz4_windows_set_dev):
    window i is elements [starts[i], starts[i] + window) of stream ids[i].
    `ids` and `starts` are contiguous int64 DEVICE tensors of equal length K,
    read by the kernels only: nothing here copies them to the host, and a call
    captured into a graph follows both at every replay.  Returns a (K, window)
    tensor of `dtype` -- with `elem_size` a uint8 tensor (K, window * elem_size)
    -- (sync=True, which reads only `result`), or (out, result) (sync=False).
    `status` (int64 device tensor, K entries): per window its byte count; -71
    for an id outside the set, a start outside [0, size - window] of its stream
    or a stream of fewer than min((window + block_size - 2) // block_size + 1,
    blocks of the largest stream) blocks (that window's part of `out` is left as
    it was); -91 for a stream whose rebuilt index failed; or the code of a
    failing block the window touches.  `out_dtype`, `scale`, `offset`: decode
    to float, as decompress_lz4_windows_dev
    (bshuf_decompress_lz4_windows_set_cvt_dev)."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, window, *ptrs):
        args = (_dptr(sset.table), sset.count, sset.max_size, es, sset.block_size, _dptr(ids), _dptr(starts), K,
                window, *ptrs, _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_windows_set_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_windows_set_dev(*args)
    return _windows_dev(call, sset.device, "set's", [("ids", ids), ("starts", starts)], dtype, window, out,
                        workspace, result, status, sync, elem_size, holds=sset.elem_size, cvt=cvt,
                        out_dtype=out_dtype)


def _ragged_dev(call, device, whose, index, dtype, max_window, out, out_offsets, pitch, workspace, result,
                status, sync, elem_size, holds=None, cvt=None, out_dtype=None):
    """What the ragged decodes of one stream and of a set share, as _windows_dev
    for the window decodes.  call(es, K, max_window, out, capacity, pitch,
    out_offsets, ws, ws_bytes, result, status) makes the library call."""
    torch = _torch()
    for name, t in index:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                and t.device == device):
            raise ValueError("%s must be a contiguous int64 tensor on the %s device" % (name, whose))
    counts = [t.numel() for _, t in index]
    if len(set(counts)) > 1:
        raise ValueError("%s need one entry per window (%s)" % (", ".join(name for name, _ in index),
                                                                ", ".join("%d" % n for n in counts)))
    K, max_window, pitch = counts[-1], int(max_window), int(pitch)
    if max_window < 0 or pitch < 0:
        raise ValueError("max_window and pitch must be >= 0, not %d and %d" % (max_window, pitch))
    per = 1 if elem_size is None else int(elem_size)  # out items per element
    if out is None:
        shape = (K, pitch * per) if pitch else (K * max_window * per,)
        own = out_dtype if cvt is not None else dtype if elem_size is None else torch.uint8
        out = torch.empty(shape, dtype=own, device=device)
    if cvt is not None:
        es = _cvt_out(cvt, out, out_dtype)
    else:
        es = out.element_size() if elem_size is None else int(elem_size)
    if holds is not None and es != holds:
        raise ValueError("the set holds %d-byte elements, not %d-byte ones" % (holds, es))
    capacity = out.numel() if cvt is not None else out.numel() * out.element_size() // es
    if cvt is not None and pitch and capacity < K * pitch:
        raise ValueError("out holds %d elements, %d rows of %d need %d" % (capacity, K, pitch, K * pitch))
    if out_offsets is None:
        out_offsets = torch.empty(K + 1, dtype=torch.int64, device=device)
    if out_offsets.dtype != torch.int64 or out_offsets.numel() < K + 1 or not out_offsets.is_contiguous():
        raise ValueError("out_offsets must be a contiguous int64 tensor of %d entries" % (K + 1))
    if status is None:
        status = torch.empty(K, dtype=torch.int64, device=device)
    if status.dtype != torch.int64 or status.numel() < K:
        raise ValueError("status must be an int64 tensor of %d entries" % K)
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    _check(call(es, K, max_window, _dptr(out), capacity, pitch, _dptr(out_offsets), ws, wsb, _dptr(result),
                _dptr(status)))
    if not sync:
        return out, out_offsets, status, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    return out, out_offsets, status


def decompress_lz4_ragged_workspace(in_nbytes, size, elem_size, nwindows, max_window, block_size=0,
                                    device=None):
    """A workspace for decompress_lz4_ragged_dev of `nwindows` windows of at
    most `max_window` elements of a stream of `in_nbytes` bytes: its size
    depends on these numbers only, never on the starts or the counts."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_ragged_dev_workspace(in_nbytes, size, elem_size, block_size, nwindows,
                                                          max_window))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def decompress_lz4_ragged_dev(buf, size, dtype, starts, counts, max_window, out=None, out_offsets=None,
                              pitch=0, block_size=0, workspace=None, result=None, status=None, offsets=None,
                              stream=None, sync=True, elem_size=None, out_dtype=None, scale=1.0, offset=0.0):
    """Ragged window decode (bshuf_decompress_lz4_ragged_dev): window i is
    elements [starts[i], starts[i] + counts[i]) of the framed stream in uint8
    device tensor `buf`, which encodes `size` elements of `dtype`.  `starts` and
    `counts` are contiguous int64 DEVICE tensors of equal length K, read by the
    kernels only; `max_window` bounds the counts and, with K, fixes the call's
    shape, so a call captured into a graph follows both tensors at every replay.
    pitch == 0: the windows land back to back in the flat `out` (allocated with
    K * max_window elements when None), window i at element out_offsets[i] --
    `out_offsets` (int64 device tensor, K + 1 entries) receives the exclusive
    scan of the good windows' counts.  pitch >= max_window: window i lands in
    row i of a (K, pitch) `out`, the rest of the row untouched.  A window with
    a count outside [0, max_window] or a start outside [0, size - count], or
    one that does not fit a packed `out`, is refused: status -71, nothing
    written.  Returns (out, out_offsets, status) (sync=True, which reads only
    `result`), or (out, out_offsets, status, result) (sync=False).  `status`
    (int64 device tensor, K entries): per window its byte count, -71, or the
    code of a failing block that holds elements of it.  `offsets`: the stream's
    block index; without it the index is rebuilt from the whole stream.
    `out_dtype`, `scale`, `offset`: decode to float, as
    decompress_lz4_windows_dev (bshuf_decompress_lz4_ragged_cvt_dev); `out`,
    its capacity, `pitch` and `out_offsets` then count elements of out_dtype,
    `status` and `result` the stream's bytes."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, max_window, outp, capacity, pitch, *ptrs):
        offp = _dptr(offsets) if offsets is not None else None
        args = (_dptr(buf), buf.numel(), int(size), es, block_size, _dptr(starts), _dptr(counts), K, max_window,
                outp, capacity, pitch, *ptrs, offp, _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_ragged_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_ragged_dev(*args)
    return _ragged_dev(call, buf.device, "stream's", [("starts", starts), ("counts", counts)], dtype,
                       max_window, out, out_offsets, pitch, workspace, result, status, sync, elem_size, cvt=cvt,
                       out_dtype=out_dtype)


def decompress_lz4_ragged_set_workspace(sset, nwindows, max_window, device=None):
    """A workspace for decompress_lz4_ragged_set_dev of `nwindows` windows of at
    most `max_window` elements over StreamSet `sset`."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_ragged_set_dev_workspace(sset.max_size, sset.elem_size, sset.block_size,
                                                              nwindows, max_window))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or sset.device)


def decompress_lz4_ragged_set_dev(sset, dtype, ids, starts, counts, max_window, out=None, out_offsets=None,
                                  pitch=0, workspace=None, result=None, status=None, stream=None, sync=True,
                                  elem_size=None, out_dtype=None, scale=1.0, offset=0.0):
    """Ragged window decode over a StreamSet (bshuf_decompress_lz4_ragged_set_dev):
    window i is elements [starts[i], starts[i] + counts[i]) of stream ids[i];
    everything else as decompress_lz4_ragged_dev.  An id outside the set refuses
    the window (-71); a stream of any number of blocks takes windows, also one
    with fewer blocks than a window of max_window elements may touch.
    `out_dtype`, `scale`, `offset`: decode to float
    (bshuf_decompress_lz4_ragged_set_cvt_dev)."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, max_window, outp, capacity, pitch, *ptrs):
        args = (_dptr(sset.table), sset.count, sset.max_size, es, sset.block_size, _dptr(ids), _dptr(starts),
                _dptr(counts), K, max_window, outp, capacity, pitch, *ptrs, _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_ragged_set_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_ragged_set_dev(*args)
    return _ragged_dev(call, sset.device, "set's", [("ids", ids), ("starts", starts), ("counts", counts)],
                       dtype, max_window, out, out_offsets, pitch, workspace, result, status, sync, elem_size,
                       holds=sset.elem_size, cvt=cvt, out_dtype=out_dtype)


def _tiles_dev(call, device, whose, index, dtype, rows, cols, pitch, out, workspace, result, status, sync,
               elem_size, holds=None, cvt=None, out_dtype=None):
    """What the tile decodes of one stream and of a set share, as _windows_dev
    for the window decodes.  `index`: (name, tensor) pairs, the device tensors
    with one entry per tile each.  call(es, K, rows, cols, pitch, out, ws,
    ws_bytes, result, status) makes the library call with these arguments of its
    own among the others and returns its code."""
    torch = _torch()
    for name, t in index:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
                and t.device == device):
            raise ValueError("%s must be a contiguous int64 tensor on the %s device" % (name, whose))
    counts = [t.numel() for _, t in index]
    if len(set(counts)) > 1:
        raise ValueError("%s need one entry per tile (%s)" % (" and ".join(name for name, _ in index),
                                                              " and ".join("%d" % n for n in counts)))
    K, rows, cols, pitch = counts[-1], int(rows), int(cols), int(pitch)
    for name, v in (("rows", rows), ("cols", cols), ("pitch", pitch)):
        if v < 0:
            raise ValueError("%s must be >= 0, not %d" % (name, v))
    if out is None:
        if cvt is not None:
            out = torch.empty((K, rows, cols), dtype=out_dtype, device=device)
        elif elem_size is None:
            out = torch.empty((K, rows, cols), dtype=dtype, device=device)
        else:
            out = torch.empty((K, rows, cols * int(elem_size)), dtype=torch.uint8, device=device)
    if cvt is not None:
        es = _cvt_out(cvt, out, out_dtype)
    else:
        es = out.element_size() if elem_size is None else int(elem_size)
    if holds is not None and es != holds:
        raise ValueError("the set holds %d-byte elements, not %d-byte ones" % (holds, es))
    per = out.element_size() if cvt is not None else es  # bytes of `out` per element
    if out.numel() * out.element_size() < K * rows * cols * per:
        raise ValueError("out holds %d bytes, the tiles need %d"
                         % (out.numel() * out.element_size(), K * rows * cols * per))
    if status is not None and (status.dtype != torch.int64 or status.numel() < K):
        raise ValueError("status must be an int64 tensor of %d entries" % K)
    if result is None:
        result = torch.empty(1, dtype=torch.int64, device=device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    stp = _dptr(status) if status is not None else None
    _check(call(es, K, rows, cols, pitch, _dptr(out), ws, wsb, _dptr(result), stp))
    if not sync:
        return out, result
    count = int(result.item())
    if count < 0:
        _fail(count)
    return out


def decompress_lz4_tiles_workspace(in_nbytes, size, elem_size, ntiles, rows, cols, pitch, block_size=0,
                                   device=None):
    """A workspace for decompress_lz4_tiles_dev of `ntiles` tiles of rows x cols
    elements at row pitch `pitch` of a stream of `in_nbytes` bytes: its size
    depends on these numbers only, never on the starts."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_tiles_dev_workspace(in_nbytes, size, elem_size, block_size, ntiles, rows,
                                                         cols, pitch))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or "cuda")


def decompress_lz4_tiles_dev(buf, size, dtype, starts, rows, cols, pitch, block_size=0, out=None,
                             workspace=None, result=None, status=None, offsets=None, stream=None,
                             sync=True, elem_size=None, out_dtype=None, scale=1.0, offset=0.0):
    """Tile decode (bshuf_decompress_lz4_tiles_dev): K = starts.numel() tiles of
    rows x cols elements each of the framed stream in uint8 device tensor `buf`,
    which encodes `size` elements of `dtype`.  Row r of tile i is elements
    [starts[i] + r * pitch, ... + cols): for a 2-D array of row length `pitch` a
    crop with its corner at (y, x) has start y * pitch + x.  `starts` is a
    contiguous int64 DEVICE tensor of flat element indices, read by the kernels
    only: nothing here copies it to the host, and a call captured into a graph
    decodes whatever starts the tensor holds at each replay.  Returns a (K,
    rows, cols) tensor of `dtype` -- with `elem_size` a uint8 tensor (K, rows,
    cols * elem_size) -- (sync=True), or (out, result) with result a 1-element
    int64 device tensor of the byte count / error code (sync=False).  `status`
    (int64 device tensor, K entries): per tile its byte count, -71 for a start
    outside [0, size - ((rows - 1) * pitch + cols)], or the code of a failing
    block that holds one of its elements; a tile with a negative status is left
    as it was in `out`, all of it.  `offsets`: the stream's block index; without
    it the index is rebuilt from the whole stream.  `out_dtype`, `scale`,
    `offset`: decode to float, as decompress_lz4_windows_dev
    (bshuf_decompress_lz4_tiles_cvt_dev): a (K, rows, cols) tensor of
    out_dtype."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, rows, cols, pitch, *ptrs):
        offp = _dptr(offsets) if offsets is not None else None
        args = (_dptr(buf), buf.numel(), int(size), es, block_size, _dptr(starts), K, rows, cols, pitch, *ptrs,
                offp, _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_tiles_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_tiles_dev(*args)
    return _tiles_dev(call, buf.device, "stream's", [("starts", starts)], dtype, rows, cols, pitch, out,
                      workspace, result, status, sync, elem_size, cvt=cvt, out_dtype=out_dtype)


def decompress_lz4_tiles_set_workspace(sset, ntiles, rows, cols, pitch, device=None):
    """A workspace for decompress_lz4_tiles_set_dev of `ntiles` tiles of rows x
    cols elements at row pitch `pitch` over StreamSet `sset`: its size depends on
    the set's largest stream, element and block size and these numbers only."""
    torch = _torch()
    n = int(lib.bshuf_decompress_lz4_tiles_set_dev_workspace(sset.max_size, sset.elem_size, sset.block_size,
                                                             ntiles, rows, cols, pitch))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device or sset.device)


def decompress_lz4_tiles_set_dev(sset, dtype, ids, starts, rows, cols, pitch, out=None, workspace=None,
                                 result=None, status=None, stream=None, sync=True, elem_size=None,
                                 out_dtype=None, scale=1.0, offset=0.0):
    """Tile decode over a StreamSet (bshuf_decompress_lz4_tiles_set_dev): row r
    of tile i is elements [starts[i] + r * pitch, ... + cols) of stream ids[i] --
    a rows x cols crop of frame ids[i] of a stack of images stored one stream
    each.  `ids` and `starts` are contiguous int64 DEVICE tensors of equal
    length K, read by the kernels only: nothing here copies them to the host,
    and a call captured into a graph follows both at every replay.  Returns a
    (K, rows, cols) tensor of `dtype` -- with `elem_size` a uint8 tensor (K,
    rows, cols * elem_size) -- (sync=True, which reads only `result`), or (out,
    result) (sync=False).  `status` (int64 device tensor, K entries): per tile
    its byte count; -71 for an id outside the set, a start outside [0, size -
    span] of its stream (span = (rows - 1) * pitch + cols) or a stream with
    fewer blocks than a group of the tile's rows decodes (that tile's part of
    `out` is left as it was); -91 for a stream whose rebuilt index failed; or
    the code of a failing block that holds one of the tile's elements, and then
    none of the tile is written.  `out_dtype`, `scale`, `offset`: decode to
    float (bshuf_decompress_lz4_tiles_set_cvt_dev)."""
    cvt = _cvt(dtype, out_dtype, scale, offset, elem_size)

    def call(es, K, rows, cols, pitch, *ptrs):
        args = (_dptr(sset.table), sset.count, sset.max_size, es, sset.block_size, _dptr(ids), _dptr(starts), K,
                rows, cols, pitch, *ptrs, _stream(stream))
        if cvt is not None:
            return lib.bshuf_decompress_lz4_tiles_set_cvt_dev(*args, ctypes.byref(cvt))
        return lib.bshuf_decompress_lz4_tiles_set_dev(*args)
    return _tiles_dev(call, sset.device, "set's", [("ids", ids), ("starts", starts)], dtype, rows, cols, pitch,
                      out, workspace, result, status, sync, elem_size, holds=sset.elem_size, cvt=cvt,
                      out_dtype=out_dtype)


def block_index_dev(buf, size, elem_size, block_size=0, workspace=None, stream=None):
    """The block index of the framed stream in uint8 device tensor `buf` for
    `size` elements of `elem_size` bytes (bshuf_lz4_block_index_dev, the
    decoder's parallel header walk): an int64 tensor of every block's byte
    offset.  Raises BshufError(-91) when the records do not tile the stream,
    -1001 when a block cannot be placed."""
    torch = _torch()
    nb = int(lib.bshuf_lz4_dev_nblocks(size, elem_size, block_size))
    offs = torch.empty(max(nb, 1), dtype=torch.int64, device=buf.device)
    status = torch.empty(1, dtype=torch.int64, device=buf.device)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    _check(lib.bshuf_lz4_block_index_dev(_dptr(buf), buf.numel(), size, elem_size, block_size, ws,
                                         wsb, _dptr(offs), _dptr(status), _stream(stream)))
    if int(status.item()) != 0:
        _fail(-91)
    if nb and bool((offs[:nb] == -1).any()):
        _fail(-1001)  # a block the walk could not place (the decoder's code for it)
    return offs[:nb]


def _ptr_array(vals):
    arr = (ctypes.c_void_p * len(vals))(*[ctypes.c_void_p(v) for v in vals])
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _size_array(vals):
    arr = (ctypes.c_size_t * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def compress_lz4_batch_dev(tensors, block_size=0, outs=None, workspace=None, offsets=None,
                           stream=None, sync=True, elem_size=None, mode="exact"):
    """bshuf_compress_lz4_batch_dev over a list of device tensors (same dtype):
    one launch per kernel for all of them.  Returns the list of framed uint8
    streams (sync=True), or (outs, results) with results a device int64 tensor
    of per-stream byte counts / error codes.  `elem_size` overrides the
    tensors' element size (as in compress_lz4_dev).  mode="fast" selects
    bshuf_compress_lz4_fast_batch_dev."""
    torch = _torch()
    fn = _mode(mode, lib.bshuf_compress_lz4_batch_dev, lib.bshuf_compress_lz4_fast_batch_dev)
    if not tensors:
        return []
    es = _elems(tensors[0], elem_size)[1]
    sizes = [_elems(t, elem_size)[0] for t in tensors]
    if outs is None:
        outs = [torch.empty(max(compress_lz4_bound(n, es, block_size), 1), dtype=torch.uint8,
                            device=t.device) for n, t in zip(sizes, tensors)]
    for t in tensors:
        if _elems(t, elem_size)[1] != es:
            raise ValueError("all tensors of a batch need the same element size")
        _dptr(t)
    results = torch.empty(len(tensors), dtype=torch.int64, device=tensors[0].device)
    pin, keep1 = _ptr_array([t.data_ptr() for t in tensors])
    pout, keep2 = _ptr_array([o.data_ptr() for o in outs])
    psz, keep3 = _size_array(sizes)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    offp = _dptr(offsets) if offsets is not None else None
    _check(fn(pin, pout, psz, len(tensors), es, block_size, ws, wsb, _dptr(results), offp,
              _stream(stream)))
    if not sync:
        return outs, results
    counts = results.cpu().tolist()
    for c in counts:
        if c < 0:
            _fail(c)
    return [o[:c] for o, c in zip(outs, counts)]


def decompress_lz4_batch_dev(bufs, shapes, dtype, block_size=0, outs=None, workspace=None,
                             stream=None, sync=True, elem_size=None, lengths=None):
    """bshuf_decompress_lz4_batch_dev: each uint8 device tensor of `bufs` is one
    whole framed stream; returns the decoded tensors (sync=True), or (outs,
    results) with per-stream consumed byte counts / error codes.  With
    `elem_size`, shapes count elem_size-byte elements and the outputs are
    uint8 tensors of their bytes.  With `lengths` (an int64 DEVICE tensor of
    len(bufs), e.g. compress_lz4_batch_dev's results with sync=False), the
    stream lengths are read on the device (bshuf_decompress_lz4_batch_dev_dlen)
    and each buffer is only its stream's capacity."""
    torch = _torch()
    if not bufs:
        return []

    def count(sh):
        c = 1
        for x in sh:
            c *= int(x)
        return c
    if outs is None:
        if elem_size is None:
            outs = [torch.empty(tuple(sh), dtype=dtype, device=b.device) for b, sh in zip(bufs, shapes)]
        else:
            outs = [torch.empty(count(sh) * int(elem_size), dtype=torch.uint8, device=b.device)
                    for b, sh in zip(bufs, shapes)]
    if elem_size is None:
        es = outs[0].element_size()
        sizes = [o.numel() for o in outs]
    else:
        es = int(elem_size)
        sizes = [count(sh) for sh in shapes]
    nbytes = [b.numel() for b in bufs]
    results = torch.empty(len(bufs), dtype=torch.int64, device=bufs[0].device)
    pin, keep1 = _ptr_array([_dptr(b).value or 0 for b in bufs])
    pout, keep2 = _ptr_array([_dptr(o).value or 0 for o in outs])
    psz, keep3 = _size_array(sizes)
    pnb, keep4 = _size_array(nbytes)
    ws = ctypes.c_void_p(workspace.data_ptr()) if workspace is not None else None
    wsb = workspace.numel() if workspace is not None else 0
    if lengths is None:
        _check(lib.bshuf_decompress_lz4_batch_dev(pin, pnb, pout, psz, len(bufs), es, block_size, ws,
                                                  wsb, _dptr(results), _stream(stream)))
    else:
        if lengths.dtype != torch.int64 or lengths.numel() < len(bufs):
            raise ValueError("lengths must be an int64 device tensor with one entry per stream")
        _check(lib.bshuf_decompress_lz4_batch_dev_dlen(pin, _dptr(lengths), pnb, pout, psz, len(bufs),
                                                       es, block_size, ws, wsb, _dptr(results),
                                                       _stream(stream)))
    if not sync:
        return outs, results
    counts = results.cpu().tolist()
    if lengths is not None:
        nbytes = lengths.reshape(-1)[: len(bufs)].cpu().tolist()
    for c, nb in zip(counts, nbytes):
        if c < 0:
            _fail(c)
        if c != nb:
            raise BshufError("Decompressed different number of bytes than input buffer size."
                             "Input buffer %d, decompressed %d." % (nb, c), c)
    return outs


def synth_fill_dev(t, gen, first=0, seed=12345, stream=None):
    """Fill tensor t with synthetic input G0 (int32 ramp), G1 (int16) or G2 (float32)."""
    _check(lib.bshuf_synth_fill_dev(_dptr(t), t.numel(), gen, first, seed, _stream(stream)))
    return t

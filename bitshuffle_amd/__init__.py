"""bitshuffle_amd -- MI355X-native bitshuffle + LZ4 (drop-in for kiyo-masui/bitshuffle).

Python mirror of the reference's module API (bitshuffle/__init__.py:24-35,
bitshuffle/ext.pyx:311-505): same function names, argument meaning and error
behaviour, backed by the HIP/gfx950 C-ABI library libbitshuffle_mi355x.so
(built in-tree by bitshuffle_amd/Makefile).  There is no CPU fallback: if the
library or a HIP device is missing, calls raise.

Host (numpy) functions
    bitshuffle(arr, block_size=0)            -> array, same shape/dtype
    bitunshuffle(arr, block_size=0)          -> array
    compress_lz4(arr, block_size=0)          -> uint8 array (framed stream)
        mode="fast" (here and in the device compress functions): the fast
        parse FAST_PARSE_VERSION -- same format, not the reference's bytes
    decompress_lz4(arr, shape, dtype, block_size=0) -> array
Device (torch CUDA/HIP tensor) functions, no host round trip
    bitshuffle_dev / bitunshuffle_dev / compress_lz4_dev / decompress_lz4_dev
    compress_lz4_batch_dev / decompress_lz4_batch_dev  (many streams per launch)
Random-access decode (device): element ranges of one stream, decoding only
the blocks they touch
    decompress_lz4_ranges_dev(buf, size, dtype, ranges, ...) -> list of tensors,
        one per (start, count) of `ranges`, views of one dense output
    decompress_lz4_range_dev(buf, size, dtype, start, count, ...) -> tensor
    decompress_lz4_ranges_workspace(in_nbytes, size, elem_size, ranges, ...)
Window decode (device): K windows of one length whose starts are a DEVICE
tensor the host never reads (replayable under graph capture)
    decompress_lz4_windows_dev(buf, size, dtype, starts, window, ...) -> (K, window)
    decompress_lz4_windows_workspace(in_nbytes, size, elem_size, nwindows, window, ...)
Window decode over a set of streams (device): window i lies in stream ids[i] at
starts[i], both DEVICE tensors; the set is built once
    lz4_stream_set_dev(bufs, sizes, elem_size, block_size=0, offsets=None, ...) -> StreamSet
    decompress_lz4_windows_set_dev(sset, dtype, ids, starts, window, ...) -> (K, window)
    decompress_lz4_windows_set_workspace(sset, nwindows, window, ...)
Tile decode (device): K crops of rows x cols elements at row pitch `pitch`, row r
of tile i being elements [starts[i] + r * pitch, ... + cols) of one stream or of
stream ids[i] of a set; rows that share blocks are decoded together, a tile with
a failing block is not written at all
    decompress_lz4_tiles_dev(buf, size, dtype, starts, rows, cols, pitch, ...) -> (K, rows, cols)
    decompress_lz4_tiles_workspace(in_nbytes, size, elem_size, ntiles, rows, cols, pitch, ...)
    decompress_lz4_tiles_set_dev(sset, dtype, ids, starts, rows, cols, pitch, ...) -> (K, rows, cols)
    decompress_lz4_tiles_set_workspace(sset, ntiles, rows, cols, pitch, ...)
Ragged window decode (device): K windows whose starts AND counts are DEVICE
tensors, bounded by max_window; packed back to back with an offsets tensor
(values + offsets), or one per row of a (K, pitch) output
    decompress_lz4_ragged_dev(buf, size, dtype, starts, counts, max_window, ...)
        -> (out, out_offsets, status)
    decompress_lz4_ragged_workspace(in_nbytes, size, elem_size, nwindows, max_window, ...)
    decompress_lz4_ragged_set_dev(sset, dtype, ids, starts, counts, max_window, ...)
    decompress_lz4_ragged_set_workspace(sset, nwindows, max_window, ...)
Decode to float (device): the six window, tile and ragged functions above take
    out_dtype=None, scale=1.0, offset=0.0
With out_dtype torch.float32, float16 or bfloat16 every element x of the stream
(dtype uint8, int8, uint16, int16, uint32, int32 or float32) lands as
out_dtype(fmaf(float32(x), scale, offset)) -- one fp32 fused multiply-add, every
rounding to nearest even -- written by the kernel that copies the decoded
elements out (bshuf_decompress_lz4_*_cvt_dev).  `out` has out_dtype and the usual
shape; status and result go on counting the stream's bytes; the workspaces are
the plain calls'.  out_dtype=None: nothing changes.
"""
from ._lib import (  # noqa: F401
    LIB_PATH,
    BshufError,
    lib,
    using_AVX2,
    using_AVX512,
    using_HIP,
    using_NEON,
    using_SSE2,
)
from .api import (  # noqa: F401
    FAST_PARSE_VERSION,
    StreamSet,
    bitshuffle,
    bitshuffle_dev,
    bitunshuffle,
    bitunshuffle_dev,
    compress_lz4,
    compress_lz4_batch_dev,
    compress_lz4_bound,
    compress_lz4_dev,
    decompress_lz4,
    decompress_lz4_batch_dev,
    decompress_lz4_dev,
    decompress_lz4_ragged_dev,
    decompress_lz4_ragged_set_dev,
    decompress_lz4_ragged_set_workspace,
    decompress_lz4_ragged_workspace,
    decompress_lz4_range_dev,
    decompress_lz4_ranges_dev,
    decompress_lz4_ranges_workspace,
    decompress_lz4_tiles_dev,
    decompress_lz4_tiles_set_dev,
    decompress_lz4_tiles_set_workspace,
    decompress_lz4_tiles_workspace,
    decompress_lz4_windows_dev,
    decompress_lz4_windows_set_dev,
    decompress_lz4_windows_set_workspace,
    decompress_lz4_windows_workspace,
    default_block_size,
    lz4_stream_set_dev,
    synth_fill_dev,
)

__version__ = "0.6.0"
__zstd__ = False

__all__ = [
    "__version__",
    "bitshuffle",
    "bitunshuffle",
    "using_NEON",
    "using_SSE2",
    "using_AVX2",
    "using_AVX512",
    "using_HIP",
    "compress_lz4",
    "decompress_lz4",
    "bitshuffle_dev",
    "bitunshuffle_dev",
    "compress_lz4_dev",
    "decompress_lz4_dev",
    "compress_lz4_batch_dev",
    "decompress_lz4_batch_dev",
    "decompress_lz4_ranges_dev",
    "decompress_lz4_range_dev",
    "decompress_lz4_ranges_workspace",
    "decompress_lz4_windows_dev",
    "decompress_lz4_windows_workspace",
    "StreamSet",
    "lz4_stream_set_dev",
    "decompress_lz4_windows_set_dev",
    "decompress_lz4_windows_set_workspace",
    "decompress_lz4_ragged_dev",
    "decompress_lz4_ragged_workspace",
    "decompress_lz4_ragged_set_dev",
    "decompress_lz4_ragged_set_workspace",
    "decompress_lz4_tiles_dev",
    "decompress_lz4_tiles_workspace",
    "decompress_lz4_tiles_set_dev",
    "decompress_lz4_tiles_set_workspace",
    "FAST_PARSE_VERSION",
]

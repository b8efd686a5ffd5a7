/*
 * bitshuffle.h -- drop-in C-ABI for bitshuffle + LZ4 (framed stream), served
 * by hand-written HIP kernels on MI355X (gfx950).
 *
 * Replaces (same names, signatures, argument meaning, return values):
 *   bshuf_compress_lz4_bound   src/bitshuffle.h:58-74  (impl src/bitshuffle.c:214-233)
 *   bshuf_compress_lz4         src/bitshuffle.h:77-98  (impl src/bitshuffle.c:236-240)
 *   bshuf_decompress_lz4       src/bitshuffle.h:101-116 (impl src/bitshuffle.c:243-247)
 * Stream format (bit-exact with the reference): for each block of block_size
 * elements (then one partial block of (size % block_size) & ~7 elements)
 *   u32 big-endian  c   ||  c bytes of LZ4 v1.10.0 block (LZ4_compress_default)
 * of the block's bit-transposed bytes, followed by (size % 8) * elem_size raw
 * bytes.  bshuf_compress_lz4 returns bytes written; bshuf_decompress_lz4
 * returns bytes CONSUMED from `in`.  ZSTD entry points are out of scope.
 */
#ifndef BITSHUFFLE_H
#define BITSHUFFLE_H

#include "bitshuffle_core.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t bshuf_compress_lz4_bound(const size_t size, const size_t elem_size, size_t block_size);

int64_t bshuf_compress_lz4(const void* in, void* out, const size_t size,
                           const size_t elem_size, size_t block_size);

int64_t bshuf_decompress_lz4(const void* in, void* out, const size_t size,
                             const size_t elem_size, size_t block_size);

/* ---- device-resident extensions (additive, not in the reference) ----
 *
 * Workspace: pass ws=NULL to let the library take it from its own device
 * memory pool (stream-ordered allocate/free per call; the pool keeps up to the
 * largest workspace requested so far mapped), or
 * pre-allocate bshuf_*_dev_workspace() bytes of device memory (must be
 * 256-byte aligned) so the call performs no allocation and can be captured
 * into a hipGraph.
 *
 * Results are written to *d_result (a DEVICE int64): bytes written (compress),
 * bytes consumed (decompress), or a negative error code.  The call itself
 * returns 0 once the work is enqueued, or a negative code for host-detected
 * argument errors.  Nothing synchronises.
 *
 * bshuf_decompress_lz4_dev needs `in_nbytes`, the number of readable bytes at
 * `in` (the reference's host API walks headers through the buffer instead;
 * on the device the block index is rebuilt in parallel from the framing and
 * in_nbytes bounds every read).  `block_offsets` (optional, may be NULL) lets
 * a caller that kept the encoder's index skip that rebuild: bshuf_compress_lz4_dev
 * fills it when non-NULL (nblocks u64 entries = byte offset of each block header).
 *
 * bshuf_decompress_lz4_dev_dlen takes the stream length as a DEVICE int64
 * (d_in_nbytes, read by the kernels when they run -- e.g. the d_result word of
 * a bshuf_compress_lz4_dev enqueued before it on the same stream), so a
 * compress -> decompress chain never waits on the host.  Like the reference's
 * bshuf_decompress_lz4 (src/bitshuffle.c:243-247, which is not told the length
 * at all), the host passes no length; in_capacity bounds every read (readable
 * bytes = min(*d_in_nbytes, in_capacity)) and sizes the workspace
 * (bshuf_decompress_lz4_dev_workspace(in_capacity, ...)).  A negative
 * *d_in_nbytes (an upstream error) is written to *d_result unchanged.
 */
size_t bshuf_compress_lz4_dev_workspace(size_t size, size_t elem_size, size_t block_size);
size_t bshuf_decompress_lz4_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                          size_t block_size);
size_t bshuf_lz4_dev_nblocks(size_t size, size_t elem_size, size_t block_size);

int64_t bshuf_compress_lz4_dev(const void* in, void* out, size_t size, size_t elem_size,
                               size_t block_size, void* ws, size_t ws_bytes,
                               int64_t* d_result, uint64_t* block_offsets, void* stream);

int64_t bshuf_decompress_lz4_dev(const void* in, size_t in_nbytes, void* out, size_t size,
                                 size_t elem_size, size_t block_size, void* ws,
                                 size_t ws_bytes, int64_t* d_result,
                                 const uint64_t* block_offsets, void* stream);
int64_t bshuf_decompress_lz4_dev_dlen(const void* in, const int64_t* d_in_nbytes, size_t in_capacity,
                                      void* out, size_t size, size_t elem_size, size_t block_size,
                                      void* ws, size_t ws_bytes, int64_t* d_result,
                                      const uint64_t* block_offsets, void* stream);

/* The block index of a framed stream alone (the decoder's parallel header walk,
 * replacing the reference's serial iochain walk, src/iochain.c:42-64): block k's
 * byte offset into block_offsets[k] (device, bshuf_lz4_dev_nblocks() entries;
 * ~0 for a block the walk could not place) and into *d_status 0 when the records
 * tile the stream exactly, nonzero otherwise (decoding would return -91).  The
 * workspace is bshuf_decompress_lz4_dev_workspace(in_nbytes, ...) bytes, or NULL
 * (library pool).  For splitting one stream's decode across devices. */
int64_t bshuf_lz4_block_index_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                  size_t block_size, void* ws, size_t ws_bytes,
                                  uint64_t* block_offsets, int64_t* d_status, void* stream);

/* ---- random-access decode: element ranges of one stream (additive) ----
 *
 * Decodes `nranges` element ranges of ONE framed stream into one dense output,
 * on the device: only the blocks a range touches are decoded.  size, elem_size
 * and block_size describe the WHOLE array the stream encodes, as for
 * bshuf_decompress_lz4_dev.  starts[] and counts[] are HOST arrays (read before
 * the call returns): range i is elements [starts[i], starts[i] + counts[i]).
 * `out` (device, any byte alignment) receives the ranges' bytes back to back in
 * list order -- range i begins at byte elem_size * (counts[0] + ... +
 * counts[i-1]) -- and nothing outside its first elem_size * sum(counts) bytes
 * is written.  Ranges may overlap, repeat, come in any order and be empty.
 *
 * block_offsets: the stream's block index (device; what bshuf_compress_lz4_dev
 * or bshuf_lz4_block_index_dev wrote), or NULL.  With an index, only the
 * records of the touched blocks are read (and the last block's header and the
 * verbatim tail when a range reaches the tail), so a corrupt block cannot
 * affect a range that does not touch it.  With NULL the index is rebuilt from
 * the whole stream first; a stream whose records do not tile it gives -91.
 *
 * *d_result (device): elem_size * sum(counts) on success, else the negative
 * code the whole decode reports for a failing block among those decoded here.
 * Returns 0 once the work is enqueued; nothing synchronises the host.  Host
 * errors: an invalid block_size as the other entries (-81), a range that does
 * not lie inside [0, size] or a workspace that is too small or not 256-byte
 * aligned -71.  The workspace is bshuf_decompress_lz4_ranges_dev_workspace(...)
 * bytes for the same arguments, or NULL (library pool). */
size_t bshuf_decompress_lz4_ranges_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                 size_t block_size, const size_t* starts,
                                                 const size_t* counts, size_t nranges);
int64_t bshuf_decompress_lz4_ranges_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                        size_t block_size, const size_t* starts, const size_t* counts,
                                        size_t nranges, void* out, void* ws, size_t ws_bytes,
                                        int64_t* d_result, const uint64_t* block_offsets, void* stream);

/* ---- window decode: fixed-length windows at device-held starts (additive) ----
 *
 * Decodes `nwindows` windows of `window` elements each of ONE framed stream.
 * size, elem_size and block_size describe the WHOLE array, as for the ranges
 * entry.  d_starts is a DEVICE array of nwindows element indices, read by the
 * kernels: window i is elements [d_starts[i], d_starts[i] + window), and its
 * window * elem_size bytes land at out + i * window * elem_size (`out`: device,
 * any byte alignment; nothing else of it is written).  Windows may overlap,
 * repeat and come in any order.  The host never sees the starts: the call
 * never waits on the host, with a caller workspace it allocates nothing, and
 * captured once into a graph it may be replayed any number of times while the
 * contents of d_starts change between replays.
 *
 * Every window decodes the same number of blocks, Mw = min((window +
 * block_size - 2) / block_size + 1, blocks of the stream), into a staging area
 * of its own and is copied from there: the workspace holds nwindows * Mw
 * staging blocks (block_size * elem_size bytes each) plus per-window and
 * per-block tables and the token positions --
 * bshuf_decompress_lz4_windows_dev_workspace(...) bytes, which depend on the
 * call's shape only, never on the starts -- or NULL (library pool).
 *
 * A start that is negative or above size - window is not decoded: that
 * window's bytes of `out` stay untouched and d_status[i] = -71.  Otherwise
 * d_status[i] (device, nwindows words, or NULL) is window * elem_size, or the
 * negative code the whole decode gives for a failing block the window touches
 * (-91 when the window reaches a verbatim tail that is not inside the stream).
 * *d_result (device): -91 when the index was rebuilt (block_offsets NULL) and
 * the records do not tile the stream; else -71 when any start was out of
 * range; else the status of the highest-numbered failing window; else nwindows
 * * window * elem_size.  block_offsets as for the ranges entry: with it, only
 * the records of touched blocks are read (and the last block's header and the
 * tail bytes when a window reaches the verbatim tail).
 *
 * Returns 0 once enqueued (nwindows == 0 or window == 0: *d_result = 0).  Host
 * errors: an invalid block_size as the other entries (-81); -71 for window >
 * size, nwindows * ((window + block_size - 2) / block_size + 1) >= 2^31, a block
 * above the LDS decoder's size (such streams: the ranges entry), a workspace
 * that is too small or not 256-byte aligned; -70 without a device. */
size_t bshuf_decompress_lz4_windows_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                  size_t block_size, size_t nwindows, size_t window);
int64_t bshuf_decompress_lz4_windows_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                         size_t block_size, const int64_t* d_starts, size_t nwindows,
                                         size_t window, void* out, void* ws, size_t ws_bytes,
                                         int64_t* d_result, int64_t* d_status,
                                         const uint64_t* block_offsets, void* stream);

/* ---- window decode over a set of streams (additive) ----
 *
 * Data is rarely one stream: an HDF5 dataset under filter 32008 is one stream
 * per chunk, bshuf_compress_lz4_batch_dev makes one per tensor.  A STREAM SET
 * is a device-resident table of `count` framed streams that share elem_size and
 * block_size, built once; the window decode over it takes, per window, the
 * index of its stream and its start, both from DEVICE arrays.
 *
 * bshuf_lz4_stream_set_dev builds the set into d_set (device, 256-byte aligned,
 * bshuf_lz4_stream_set_dev_bytes(...) bytes).  ins[], in_nbytes[], sizes[] and
 * block_offsets[] are HOST arrays of device pointers / sizes, as for the batch
 * entries; block_offsets is NULL, or holds per stream that stream's block index
 * or NULL.  A stream without a supplied index gets its index rebuilt HERE, once,
 * into the set's own memory; d_status[s] (device, count words) is then 0, or
 * -91 when that stream's records do not tile it (every window in it will report
 * -91; the other streams are not affected).  The set holds POINTERS into the
 * streams and into every supplied index: they must stay alive and unchanged in
 * place for as long as the set is used (their contents may change between
 * calls only where the index stays right).  d_set layout: a header (magic
 * word, count, elem_size, block_size, the largest stream's block count nb_max
 * and the index of one stream with that many blocks), one 64-byte record per
 * stream at byte 256 (stream pointer and length, index pointer, block count,
 * tail bytes, largest record, element count, error word), then the rebuilt
 * indexes.  The workspace (bshuf_lz4_stream_set_dev_workspace(...) bytes, or
 * NULL: library pool) is only needed until the build has run.  count == 0 is
 * valid: a set no window can address.  Host errors: -81 for an invalid
 * block_size; -71 for a block above the LDS decoder's size, a set_bytes or
 * ws_bytes that is too small, d_set or ws not 256-byte aligned, 2^31 or more
 * blocks or index chunks in all; -70 without a device.  The two size functions
 * return 0 for arguments the build refuses.
 *
 * bshuf_decompress_lz4_windows_set_dev decodes nwindows windows of `window`
 * elements: window i is elements [d_starts[i], d_starts[i] + window) of stream
 * d_ids[i], and lands at out + i * window * elem_size, as in the single-stream
 * entry.  count, elem_size and block_size are the set's; max_size is the element
 * count of its largest stream.  Every window decodes Mw = min((window +
 * block_size - 2) / block_size + 1, nb_max) consecutive blocks of its stream
 * into a staging area of its own, so the call's launches and its workspace
 * (bshuf_decompress_lz4_windows_set_dev_workspace(...) bytes, or NULL) depend on
 * count, max_size, elem_size, block_size, nwindows and window alone: the host
 * never reads ids or starts, nothing is uploaded, nothing synchronises, and a
 * call captured into a graph follows both arrays at every replay.
 *
 * d_status[i] (device, nwindows words, or NULL): window * elem_size; or -71 for
 * a window that is not decoded (its bytes of `out` stay untouched) -- d_ids[i]
 * outside [0, count), window above that stream's size, d_starts[i] outside [0,
 * size - window], or a stream of FEWER THAN Mw BLOCKS: such a stream takes no
 * window of this length (one shape per call; decode it whole, or with the
 * single-stream entry); or -91 for a stream whose rebuilt index failed; or the
 * code of the highest failing block among those that hold the window's
 * elements; or -91 when the window reaches a verbatim tail that is not inside
 * its stream.  *d_result: -71 when any window was not decoded, else the status
 * of the highest-numbered failing window, else nwindows * window * elem_size.
 * When the set's header does not carry the call's count, elem_size, block_size
 * and nb_max, every window is -71 and no stream is read.
 *
 * Returns 0 once enqueued (nwindows == 0 or window == 0: *d_result = 0).  Host
 * errors: -81; -71 for window > max_size, nwindows * ((window + block_size - 2)
 * / block_size + 1) >= 2^31, a block above the LDS decoder's size, a workspace
 * that is too small or not 256-byte aligned, d_set NULL or not 256-byte
 * aligned; -70 without a device. */
size_t bshuf_lz4_stream_set_dev_bytes(const size_t* sizes, size_t count, size_t elem_size, size_t block_size);
size_t bshuf_lz4_stream_set_dev_workspace(const size_t* in_nbytes, const size_t* sizes, size_t count,
                                          size_t elem_size, size_t block_size);
int64_t bshuf_lz4_stream_set_dev(const void* const* ins, const size_t* in_nbytes, const size_t* sizes,
                                 size_t count, size_t elem_size, size_t block_size,
                                 const uint64_t* const* block_offsets, void* d_set, size_t set_bytes,
                                 void* ws, size_t ws_bytes, int64_t* d_status, void* stream);
size_t bshuf_decompress_lz4_windows_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                      size_t nwindows, size_t window);
int64_t bshuf_decompress_lz4_windows_set_dev(const void* d_set, size_t count, size_t max_size,
                                             size_t elem_size, size_t block_size, const int64_t* d_ids,
                                             const int64_t* d_starts, size_t nwindows, size_t window,
                                             void* out, void* ws, size_t ws_bytes, int64_t* d_result,
                                             int64_t* d_status, void* stream);

/* ---- ragged window decode: device-held starts AND lengths (additive) ----
 *
 * Decodes nwindows windows whose lengths differ and live in device memory like
 * their starts: window i is elements [d_starts[i], d_starts[i] + d_counts[i]) of
 * ONE framed stream (bshuf_decompress_lz4_ragged_dev; in .. block_size and
 * block_offsets as for the window entry) or of stream d_ids[i] of a stream set
 * (bshuf_decompress_lz4_ragged_set_dev; d_set, count, max_size as for the window
 * entry over a set).  d_starts, d_counts (and d_ids) are DEVICE int64 arrays of
 * nwindows words that the host never reads.  max_window, a bound on the counts,
 * nwindows, out_capacity and out_pitch (both in elements) are host values; with
 * the stream (or count, max_size) they fix the workspace
 * (bshuf_decompress_lz4_ragged[_set]_dev_workspace(...) bytes, or NULL) and the
 * launch sequence: one linear chain on `stream`, nothing uploaded, nothing
 * synchronised, and a call captured into a graph follows the arrays at every
 * replay.
 *
 * Window i is GOOD when 0 <= d_counts[i] <= max_window and 0 <= d_starts[i] <=
 * size - d_counts[i], size being its stream's element count -- over a set,
 * d_ids[i] must also name one of its streams, which may have any number of
 * blocks.  A good window of count 0 has status 0 and writes nothing.  Any other
 * window is REFUSED: status -71, nothing written.  Over a set whose header does
 * not carry the call's count, elem_size, block_size and nb_max, every window is
 * refused and no stream is read.
 *
 * Packed output (out_pitch == 0): window i lands at out + off[i] * elem_size,
 * off being the exclusive scan of eff[i] = d_counts[i] for a good window and 0
 * for a refused one; off[0 .. nwindows] is written to d_out_offsets (device,
 * nwindows + 1 words, required): values + offsets, as a jagged tensor has them.
 * The offsets depend on starts, counts and ids only: a window whose block fails
 * to decode keeps its room, and its bytes stay untouched.  A good window with
 * off[i] + d_counts[i] > out_capacity is not written and gets -71 (the offsets
 * stay the plain scan); nothing is written at or behind out + out_capacity *
 * elem_size.  Padded output (out_pitch >= max_window): window i lands at out +
 * i * out_pitch * elem_size, the rest of its row stays untouched, out_capacity
 * must be at least nwindows * out_pitch, and d_out_offsets may be NULL (given,
 * it still receives the scan).
 *
 * d_status[i] (device, nwindows words, or NULL): d_counts[i] * elem_size; or
 * -71 for a refused window; or -91 for a stream of a set whose rebuilt index
 * failed; or the code of the highest failing block among those that hold the
 * window's elements -- a neighbouring block's failure is not the window's; or
 * -91 when the window reaches a verbatim tail that is not inside its stream.
 * *d_result: -91 for a bad rebuilt index, else -71 when any window was refused,
 * else the status of the highest-numbered failing window, else the bytes
 * written, off[nwindows] * elem_size.
 *
 * Returns 0 once enqueued (nwindows == 0 or max_window == 0: *d_result = 0 and
 * d_out_offsets, when given, zero-filled).  Host errors: -81; -71 for
 * max_window > size (max_size), nwindows * ((max_window + block_size - 2) /
 * block_size + 1) >= 2^31, a block above the LDS decoder's size, 0 < out_pitch <
 * max_window, out_capacity < nwindows * out_pitch, out_pitch == 0 without
 * d_out_offsets, a workspace that is too small or not 256-byte aligned, d_set
 * NULL or not 256-byte aligned; -70 without a device. */
size_t bshuf_decompress_lz4_ragged_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                 size_t block_size, size_t nwindows, size_t max_window);
int64_t bshuf_decompress_lz4_ragged_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                        size_t block_size, const int64_t* d_starts, const int64_t* d_counts,
                                        size_t nwindows, size_t max_window, void* out, size_t out_capacity,
                                        size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                        int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                                        void* stream);
size_t bshuf_decompress_lz4_ragged_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                     size_t nwindows, size_t max_window);
int64_t bshuf_decompress_lz4_ragged_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                            size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                            const int64_t* d_counts, size_t nwindows, size_t max_window,
                                            void* out, size_t out_capacity, size_t out_pitch,
                                            int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                            int64_t* d_result, int64_t* d_status, void* stream);

/* ---- tile decode: rows x cols crops at device-held corners (additive) ----
 *
 * Decodes `ntiles` tiles of rows x cols elements each, of ONE framed stream
 * (bshuf_decompress_lz4_tiles_dev) or each of a stream of a stream set
 * (bshuf_decompress_lz4_tiles_set_dev; d_set, count, max_size as for the window
 * entry over a set).  The indices are flat, as for windows, and the array's
 * shape is the caller's business: for a 2-D array of row length `pitch` a tile
 * with its corner at (y, x) has start = y * pitch + x; for a stack of planes add
 * the plane's offset.  d_starts (and d_ids) are DEVICE arrays of ntiles words,
 * read by the kernels: row r of tile i is elements [d_starts[i] + r * pitch, ...
 * + cols) of the stream (of stream d_ids[i]), and its cols * elem_size bytes
 * land at out + ((i * rows + r) * cols) * elem_size (`out`: device, any byte
 * alignment; nothing else of it is written).  The host never sees ids or
 * starts: nothing is uploaded or read back, with a caller workspace nothing is
 * allocated, the launches are one linear sequence on `stream`, and a call
 * captured into a graph follows the arrays at every replay.
 *
 * With span = (rows - 1) * pitch + cols, every tile is cut into G = ceil(rows /
 * rg) groups of rg consecutive rows (the last may hold fewer), and every group
 * decodes Mg = min(((rg - 1) * pitch + cols + block_size - 2) / block_size + 1,
 * blocks of the stream -- over a set: of its largest stream) consecutive blocks
 * into a staging area of its own, from which its rows are copied.  rg is the one
 * in 1..rows with the smallest G * Mg (of equal ones the largest): rows that
 * share blocks are decoded together, rows that lie blocks apart are not
 * connected by the blocks between them.  The workspace
 * (bshuf_decompress_lz4_tiles_dev_workspace(...) /
 * bshuf_decompress_lz4_tiles_set_dev_workspace(...) bytes, or NULL: library
 * pool) holds ntiles * G staging areas of Mg blocks, per-tile, per-group and
 * per-block tables and the token positions; its size depends on the arguments
 * of these two functions alone.
 *
 * A tile is BAD when its start is outside [0, size - span]; over a set also
 * when d_ids[i] is outside [0, count), span is above that stream's size, or the
 * stream has fewer than Mg blocks (the window entry's rule).  A bad tile's
 * bytes of `out` stay untouched.  d_status[i] (device, ntiles words, or NULL)
 * is the first of these that applies: -71 for a bad tile; -91 (set) when the
 * stream's rebuilt index failed; the code of the highest failing block, in
 * stream order, among those that hold an element of the tile (blocks the tile
 * merely lies between do not count: with an index supplied, a corrupt block no
 * row touches does not fail the tile); -91 when a row reaches a verbatim tail
 * that is not inside the stream; else rows * cols * elem_size.  A tile with a
 * negative status is not written at all, not even its good rows.  *d_result
 * (device) as for the window entries: -91 for a bad rebuilt index (single
 * stream); else -71 when any tile was bad; else the status of the
 * highest-numbered failing tile; else ntiles * rows * cols * elem_size.
 *
 * Returns 0 once enqueued (ntiles, rows or cols == 0: *d_result = 0, nothing is
 * decoded).  Host errors: -81 for an invalid block_size; -71 for pitch < cols,
 * span > size (set: > max_size), a block above the LDS decoder's size, ntiles *
 * G * Mg >= 2^31 or ntiles * G >= 2^31, a workspace that is too small or not
 * 256-byte aligned, d_set NULL or not 256-byte aligned; -70 without a device.
 * The workspace functions return 0 for arguments the calls refuse. */
size_t bshuf_decompress_lz4_tiles_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                size_t block_size, size_t ntiles, size_t rows, size_t cols,
                                                size_t pitch);
int64_t bshuf_decompress_lz4_tiles_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                       size_t block_size, const int64_t* d_starts, size_t ntiles, size_t rows,
                                       size_t cols, size_t pitch, void* out, void* ws, size_t ws_bytes,
                                       int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                                       void* stream);
size_t bshuf_decompress_lz4_tiles_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                    size_t ntiles, size_t rows, size_t cols, size_t pitch);
int64_t bshuf_decompress_lz4_tiles_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                           size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                           size_t ntiles, size_t rows, size_t cols, size_t pitch, void* out,
                                           void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                           void* stream);

/* ---- decode to float: the window, ragged and tile decodes with a fused cast,
 * scale and offset (additive) ----
 *
 * Each of the six entries above has a converting twin, *_cvt_dev, with the same
 * arguments and a trailing `const bshuf_cvt* cvt` (a HOST pointer, read during
 * the call; scale and offset become kernel arguments, so a captured call keeps
 * them).  An element x of the stream lands in `out` as
 *
 *     y32 = fmaf((float)x, scale, offset)   one fp32 fused multiply-add
 *     y   = y32                             dst BSHUF_CVT_F32
 *         = (half)y32 / (bfloat16)y32       dst BSHUF_CVT_F16 / BSHUF_CVT_BF16
 *
 * every conversion rounding to nearest even, (float)x being the identity for a
 * float source, a 16-bit result overflowing to infinity.  cvt->src names the
 * stream's element type and must have elem_size bytes (so elem_size is 1, 2 or
 * 4); cvt->dst names the type of `out`.
 *
 * `out`, out_capacity, out_pitch and the d_out_offsets are in DESTINATION
 * elements: window i lands at out + i * window * sizeof(dst), row r of tile i at
 * out + ((i * rows + r) * cols) * sizeof(dst), a ragged window at out + off[i] *
 * sizeof(dst) (or i * out_pitch), and `out` must be aligned to sizeof(dst).  A
 * window or tile that the plain call would not write leaves its
 * destination-sized slice of `out` untouched.  Everything else is the plain
 * entry's: which windows and tiles are bad, d_status and *d_result -- which go
 * on counting SOURCE bytes (window * elem_size, rows * cols * elem_size, off[K]
 * * elem_size), so a caller's checks do not change -- the host errors, the
 * capture rules and the workspace, which the plain entry's _workspace function
 * sizes.  Only the kernel that copies the decoded elements out differs.
 *
 * Host errors of their own, all -71 with nothing enqueued: cvt NULL, a kind
 * that is none of the ones below, a source kind whose size is not elem_size
 * (every elem_size but 1, 2 and 4), an `out` not aligned to sizeof(dst). */
typedef struct bshuf_cvt {
    int32_t src, dst;    /* BSHUF_CVT_* source kind, destination kind */
    float scale, offset;
} bshuf_cvt;
enum { /* source kinds */
    BSHUF_CVT_U8, BSHUF_CVT_I8, BSHUF_CVT_U16, BSHUF_CVT_I16, BSHUF_CVT_U32, BSHUF_CVT_I32, BSHUF_CVT_F32_SRC
};
enum { /* destination kinds */
    BSHUF_CVT_F32, BSHUF_CVT_F16, BSHUF_CVT_BF16
};
int64_t bshuf_decompress_lz4_windows_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                             size_t block_size, const int64_t* d_starts, size_t nwindows,
                                             size_t window, void* out, void* ws, size_t ws_bytes,
                                             int64_t* d_result, int64_t* d_status,
                                             const uint64_t* block_offsets, void* stream,
                                             const bshuf_cvt* cvt);
int64_t bshuf_decompress_lz4_windows_set_cvt_dev(const void* d_set, size_t count, size_t max_size,
                                                 size_t elem_size, size_t block_size, const int64_t* d_ids,
                                                 const int64_t* d_starts, size_t nwindows, size_t window,
                                                 void* out, void* ws, size_t ws_bytes, int64_t* d_result,
                                                 int64_t* d_status, void* stream, const bshuf_cvt* cvt);
int64_t bshuf_decompress_lz4_ragged_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                            size_t block_size, const int64_t* d_starts, const int64_t* d_counts,
                                            size_t nwindows, size_t max_window, void* out, size_t out_capacity,
                                            size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                            int64_t* d_result, int64_t* d_status,
                                            const uint64_t* block_offsets, void* stream, const bshuf_cvt* cvt);
int64_t bshuf_decompress_lz4_ragged_set_cvt_dev(const void* d_set, size_t count, size_t max_size,
                                                size_t elem_size, size_t block_size, const int64_t* d_ids,
                                                const int64_t* d_starts, const int64_t* d_counts,
                                                size_t nwindows, size_t max_window, void* out,
                                                size_t out_capacity, size_t out_pitch, int64_t* d_out_offsets,
                                                void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                                void* stream, const bshuf_cvt* cvt);
int64_t bshuf_decompress_lz4_tiles_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                           size_t block_size, const int64_t* d_starts, size_t ntiles,
                                           size_t rows, size_t cols, size_t pitch, void* out, void* ws,
                                           size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                           const uint64_t* block_offsets, void* stream, const bshuf_cvt* cvt);
int64_t bshuf_decompress_lz4_tiles_set_cvt_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                               size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                               size_t ntiles, size_t rows, size_t cols, size_t pitch, void* out,
                                               void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                               void* stream, const bshuf_cvt* cvt);

/* ---- batched device entry points (additive) ----
 *
 * `count` independent framed streams per call, all with the same elem_size and
 * block_size, each with its own (device) input, output and size; one launch
 * of each kernel covers every block of every stream (the OpenMP block loop of
 * src/bitshuffle_core.c:1899-1907, widened to many buffers).  in[], out[],
 * sizes[] and in_nbytes[] are HOST arrays of device pointers / sizes;
 * d_results is a DEVICE array of `count` int64: per stream, bytes written
 * (compress) or consumed (decompress), or that stream's negative error code.
 * A corrupt stream never affects the others.  block_offsets (optional,
 * device, one u64 per block of the batch in stream order): each block's
 * header offset inside its own stream.  The per-stream table travels through a
 * per-thread pinned buffer; nothing synchronises the host.  Batches that run
 * one stream at a time (blocks above the LDS kernels' size; encode: streams
 * that need both LZ4 table types) take each stream through the caller's
 * workspace in turn: the _workspace functions return the largest single
 * stream's need for them, and with a workspace nothing is allocated.  (These
 * batches used to ignore `ws` and take pool memory: a workspace smaller than
 * the _workspace function now returns is refused with -71 for them too.)
 */
size_t bshuf_compress_lz4_batch_dev_workspace(const size_t* sizes, size_t count, size_t elem_size,
                                              size_t block_size);
int64_t bshuf_compress_lz4_batch_dev(const void* const* in, void* const* out, const size_t* sizes,
                                     size_t count, size_t elem_size, size_t block_size, void* ws,
                                     size_t ws_bytes, int64_t* d_results, uint64_t* block_offsets,
                                     void* stream);
size_t bshuf_decompress_lz4_batch_dev_workspace(const size_t* in_nbytes, const size_t* sizes,
                                                size_t count, size_t elem_size, size_t block_size);
int64_t bshuf_decompress_lz4_batch_dev(const void* const* in, const size_t* in_nbytes,
                                       void* const* out, const size_t* sizes, size_t count,
                                       size_t elem_size, size_t block_size, void* ws,
                                       size_t ws_bytes, int64_t* d_results, void* stream);
/* The same with the stream lengths as a DEVICE array d_in_nbytes[count] (e.g.
 * the d_results of a bshuf_compress_lz4_batch_dev before it on the stream);
 * in_capacity[] (host) bounds each stream's reads and sizes the workspace
 * (bshuf_decompress_lz4_batch_dev_workspace(in_capacity, ...)).  A negative
 * length is written to that stream's result unchanged. */
int64_t bshuf_decompress_lz4_batch_dev_dlen(const void* const* in, const int64_t* d_in_nbytes,
                                            const size_t* in_capacity, void* const* out,
                                            const size_t* sizes, size_t count, size_t elem_size,
                                            size_t block_size, void* ws, size_t ws_bytes,
                                            int64_t* d_results, void* stream);

/* ---- fast encode mode (additive, opt-in): "fast parse v1" ----
 *
 * The same framed bitshuffle/LZ4 stream as the entries above -- block
 * splitting, partial last block, verbatim tail, error codes, workspaces
 * (bshuf_compress_lz4_dev_workspace / _batch_dev_workspace), output bound
 * (bshuf_compress_lz4_bound) and stream semantics -- and every bitshuffle/LZ4
 * reader decodes it, but each block's LZ4 payload comes from a parse that
 * looks for matches only at the distances 1, 2, 3, 4, 8, P and 2P (P = bytes
 * per bit plane of the block), not from the reference's hash-table parse: the
 * bytes differ from the reference encoder's ("fast parse v1").  The
 * stream is a pure function of (input, elem_size, block_size).  Blocks above
 * 65536 bytes take the exact parse: such a stream equals the exact one.
 * bshuf_lz4_fast_version() names the parse rule (1). */
int bshuf_lz4_fast_version(void);
int64_t bshuf_compress_lz4_fast(const void* in, void* out, const size_t size,
                                const size_t elem_size, size_t block_size);
int64_t bshuf_compress_lz4_fast_dev(const void* in, void* out, size_t size, size_t elem_size,
                                    size_t block_size, void* ws, size_t ws_bytes,
                                    int64_t* d_result, uint64_t* block_offsets, void* stream);
int64_t bshuf_compress_lz4_fast_batch_dev(const void* const* in, void* const* out,
                                          const size_t* sizes, size_t count, size_t elem_size,
                                          size_t block_size, void* ws, size_t ws_bytes,
                                          int64_t* d_results, uint64_t* block_offsets,
                                          void* stream);

/* Synthetic benchmark inputs of SURVEY.md 8(d), generated on the device
 * (counter based, identical to the CPU definition): gen 0 = int32 ramp,
 * 1 = int16 correlated noise (G1), 2 = float32 smooth field (G2). */
int64_t bshuf_synth_fill_dev(void* out, size_t n_elem, int gen, uint64_t first,
                             uint64_t seed, void* stream);

/* Per-kernel timing (HIP events on each kernel's launch stream), for
 * benchmarks: enable, run, then collect "name count total_ms" lines.
 * bshuf_prof_collect returns the buffer size needed and resets. */
void bshuf_prof_enable(int on);
/* Times only the kernel of this name (NULL: every kernel). */
void bshuf_prof_only(const char* name);
/* Selects, for the CALLING THREAD only, an alternative kernel variant for A/B
 * measurements: 0 default, 2 inline LZ4 emitter, 4 one-group-per-lane
 * transpose, 8 re-test table lookup by lane 0's returning exchange, decoder
 * record access 16 from global memory with a two-blocks-ahead touch / 32
 * without it / 64 staged in an LDS buffer of its own (default: in place at the
 * end of the block's LDS buffer), 128 insert/read-back search window.  Every
 * accepted variant produces identical bytes; anything else is rejected with -71. */
int bshuf_set_variant(int v);
size_t bshuf_prof_collect(char* buf, size_t len);

/* Host-pointer path internals (additive).  bshuf_host_poison fills every
 * cached device buffer and pinned staging slot of the CALLING thread with
 * `byte`, so a test can start the next host call from poisoned state.
 * bshuf_host_xfer_stats: out2[0] = staged pieces moved by the transfer
 * kernels, out2[1] = pieces whose completion event fired before all of their
 * flag words were set (the host waited for the flags). */
int64_t bshuf_host_poison(int byte);
void bshuf_host_xfer_stats(uint64_t* out2);

#ifdef __cplusplus
}
#endif

#endif /* BITSHUFFLE_H */

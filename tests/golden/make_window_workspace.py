"""Recorder of tests/golden/window_workspace.json: what the workspace-size
functions of the range decode, the two window decodes and the stream set return
over a grid of call shapes.  None of them touches a device.  The file pins the
workspace layouts byte for byte (tests/test_window_workspace.py): record it from
a build whose layouts are known to be right, before a change that must not move
them.  Run:  python tests/golden/make_window_workspace.py

The file holds the grid's axes and, per function, the values in the order of
`walk` below; the test imports `walk` from here, so the two cannot disagree."""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "window_workspace.json")

GRID = {
    "elem_sizes": [1, 2, 3, 8],
    "block_sizes": [0, 64, 4096],
    # nothing, a tail alone, three blocks + a partial one + a tail (at block 64), ...
    "sizes": [0, 5, 3 * 64 + 40 + 5, 12000, 3 * 2 ** 20 + 4096 + 1000 + 5],
    # stream lengths: next to nothing (the shared token-position area is the
    # smaller one), the bound of the size, and three times that and a bit (the
    # private areas are, for few windows or ranges)
    "in_nbytes": [16, "bound", "3*bound+1000"],
    "K": [0, 1, 3, 4096],
    "windows": [0, 1, 29, 65, 65536],
    # blocks above the LDS decoder's size: (elem_size, block_size); the window
    # decodes and the stream set refuse them, the range decode does not
    "large_blocks": [[2, 98304], [8, 16384]],
    # sets of streams: sizes, and each stream's length as in "in_nbytes"
    "sets": [[], [0], [5], [237, 128, 5, 391, 88], [12000, 5, 10000], [3 * 2 ** 20 + 5101, 237, 12000]],
}


def ranges_of(size):
    """The range lists of a stream of `size` elements: none, empty ones, the
    whole stream, single elements, ranges that end inside the tail, overlapping
    and repeated ones, many short ones, and one that leaves the stream."""
    third = size // 3
    lists = [[], [(0, 0), (size, 0)], [(0, size)], [(size, 1)], [(size + 1, 0)]]
    if size:
        lists += [[(0, 1), (size - 1, 1), (size // 2, 1)],
                  [(third, size - third), (third, size - third), (0, min(size, 70))],
                  [(i * (size // 64 + 1) % size, min(29, size - i * (size // 64 + 1) % size)) for i in range(64)],
                  [(1, size - 1), (size - min(size, 9), min(size, 9))]]
    return lists


def sizes_array(vals):
    arr = (ctypes.c_size_t * max(len(vals), 1))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def length(lib, mode, size, E, block):
    bound = int(lib.bshuf_compress_lz4_bound(size, E, block))
    return {"bound": bound, "3*bound+1000": 3 * bound + 1000}.get(mode, mode)


def walk(lib, grid):
    """{function: [values]} of the library `lib` over `grid`."""
    out = {"ranges": [], "windows": [], "windows_set": [], "set_workspace": [], "set_bytes": []}
    shapes = list(itertools.product(grid["elem_sizes"], grid["block_sizes"])) + [tuple(x) for x in grid["large_blocks"]]
    for E, block in shapes:
        for size in grid["sizes"]:
            for mode in grid["in_nbytes"]:
                n = length(lib, mode, size, E, block)
                for ranges in ranges_of(size):
                    ps, k1 = sizes_array([r[0] for r in ranges])
                    pc, k2 = sizes_array([r[1] for r in ranges])
                    out["ranges"].append(int(lib.bshuf_decompress_lz4_ranges_dev_workspace(
                        n, size, E, block, ps, pc, len(ranges))))
                for K, window in itertools.product(grid["K"], grid["windows"]):
                    out["windows"].append(int(lib.bshuf_decompress_lz4_windows_dev_workspace(
                        n, size, E, block, K, window)))
            for K, window in itertools.product(grid["K"], grid["windows"]):
                out["windows_set"].append(int(lib.bshuf_decompress_lz4_windows_set_dev_workspace(
                    size, E, block, K, window)))
        for sizes in grid["sets"]:
            psz, k3 = sizes_array(sizes)
            out["set_bytes"].append(int(lib.bshuf_lz4_stream_set_dev_bytes(psz, len(sizes), E, block)))
            for mode in grid["in_nbytes"]:
                pnb, k4 = sizes_array([length(lib, mode, s, E, block) for s in sizes])
                out["set_workspace"].append(int(lib.bshuf_lz4_stream_set_dev_workspace(
                    pnb, psz, len(sizes), E, block)))
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import bitshuffle_amd

    values = walk(bitshuffle_amd.lib, GRID)
    with open(PATH, "w") as f:
        json.dump({"grid": GRID, "values": values}, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in values.items()}, os.path.getsize(PATH), "bytes")

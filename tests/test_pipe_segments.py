"""The segment bounds of the pipelined encode (bitshuffle_amd/csrc/pipe_segments.h
via libbshuf_hostcheck.so): for every schedule the launcher can run, the
segments of a call of nb blocks are monotone, start at 0, end at nb and cover
[0, nb) exactly; a segment is empty only where the launcher skips it (f1 == f0),
which happens only for calls shorter than the schedule is fine."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HOSTCHECK):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"), HOSTCHECK])
    lib = ctypes.CDLL(HOSTCHECK)
    lib.bshuf_hostcheck_pipe_seg_bound.restype = ctypes.c_int64
    lib.bshuf_hostcheck_pipe_seg_bound.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return lib


def bounds(lib, nb, schedule):
    n = lib.bshuf_hostcheck_pipe_seg_count(schedule)
    return [lib.bshuf_hostcheck_pipe_seg_bound(nb, schedule, i) for i in range(n + 1)]


def sizes(lib):
    """Per schedule: the block counts the issue names, and its own segment count."""
    out = []
    for sched in range(lib.bshuf_hostcheck_pipe_schedules()):
        segs = lib.bshuf_hostcheck_pipe_seg_count(sched)
        for nb in (0, 1, segs - 1, segs, 65536, 65541, 2 ** 31 - 1):
            out.append((sched, nb))
    return out


def test_schedules_exist(lib):
    n = lib.bshuf_hostcheck_pipe_schedules()
    assert n >= 2
    counts = [lib.bshuf_hostcheck_pipe_seg_count(s) for s in range(n)]
    assert counts[0] == 8                                   # eight equal segments
    assert max(counts) == lib.bshuf_hostcheck_pipe_segs_max()  # events and ticket sets are sized by it


def test_bounds_cover_every_block_once(lib):
    for sched, nb in sizes(lib):
        b = bounds(lib, nb, sched)
        assert b[0] == 0 and b[-1] == nb, (sched, nb, b)
        assert all(x <= y for x, y in zip(b, b[1:])), (sched, nb, b)
        # monotone bounds from 0 to nb: consecutive half-open segments, their
        # union is [0, nb) and no two overlap; spelt out for the small sizes
        if nb <= 70000:
            seen = [0] * nb
            for f0, f1 in zip(b, b[1:]):
                for k in range(f0, f1):
                    seen[k] += 1
            assert all(c == 1 for c in seen), (sched, nb)
        else:
            assert sum(f1 - f0 for f0, f1 in zip(b, b[1:])) == nb


def test_empty_segments_only_in_calls_the_launcher_skips_them_for(lib):
    for sched, nb in sizes(lib):
        b = bounds(lib, nb, sched)
        empty = [i for i, (f0, f1) in enumerate(zip(b, b[1:])) if f1 == f0]
        # from 32 blocks on (the schedules' finest step is 1/32) no segment is
        # empty; the pipelined path starts at 65,536 blocks, and skips f1 == f0
        if nb >= 32:
            assert not empty, (sched, nb, b)
        else:
            assert len(empty) >= len(b) - 1 - nb, (sched, nb, b)


def test_out_of_range_indices_clamp(lib):
    for sched in range(lib.bshuf_hostcheck_pipe_schedules()):
        n = lib.bshuf_hostcheck_pipe_seg_count(sched)
        assert lib.bshuf_hostcheck_pipe_seg_bound(1000, sched, -1) == 0
        assert lib.bshuf_hostcheck_pipe_seg_bound(1000, sched, n + 3) == 1000


def test_equal_schedule_is_eighths(lib):
    for nb in (65536, 65541, 524288, 2 ** 31 - 1, 12345677):
        assert bounds(lib, nb, 0) == [nb * i // 8 for i in range(9)]


def test_tapered_schedule_ends_in_a_thirty_second(lib):
    nb = 524288
    b = bounds(lib, nb, 1)
    assert [f1 - f0 for f0, f1 in zip(b, b[1:])] == [nb // 8] * 7 + [nb // 16, nb // 32, nb // 32]

"""CPU checks of ticket stealing between the shards of a persistent launch's
block counters (bitshuffle_amd/csrc/ticket_steal.h via libbshuf_hostcheck.so;
the scheme: csrc/bshuf_dev.h, struct Tickets):

* the per-shard ticket limit against a brute-force count;
* the victim choice (most remaining, ties to the nearest shard behind the
  wave's own, none when nothing is left) on every small `remaining` vector;
* a simulation of the scheme on top of those functions, with waves whose
  memory operations interleave at random: every block is taken exactly once,
  every wave ends, no wave makes more than kTicketShards failed draws, and a
  pending ticket of an abandoned shard is never turned into a block.
"""
import ctypes
import heapq
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HOSTCHECK):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"),
                               HOSTCHECK])
    lib = ctypes.CDLL(HOSTCHECK)
    lib.bshuf_hostcheck_ticket_shards.restype = ctypes.c_int
    lib.bshuf_hostcheck_ticket_limit.restype = ctypes.c_int64
    lib.bshuf_hostcheck_ticket_limit.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_int]
    lib.bshuf_hostcheck_ticket_remaining.restype = ctypes.c_uint32
    lib.bshuf_hostcheck_ticket_remaining.argtypes = [ctypes.c_int64, ctypes.c_uint32]
    lib.bshuf_hostcheck_ticket_victim.restype = ctypes.c_int
    lib.bshuf_hostcheck_ticket_victim.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def S(lib):
    s = lib.bshuf_hostcheck_ticket_shards()
    assert s == 8
    return s


def victim(lib, S, remaining, own):
    arr = (ctypes.c_uint32 * S)(*remaining)
    return lib.bshuf_hostcheck_ticket_victim(arr, own)


def test_per_shard_limit_against_brute_force(lib, S):
    for first in (0, 1, 5, 1000, (1 << 31) - 100):
        for G in range(1, 21):
            for extra in range(0, 41):
                end = first + G + extra
                for c in range(S):
                    brute = sum(1 for t in range(extra + 1) if first + G + S * t + c < end)
                    assert lib.bshuf_hostcheck_ticket_limit(first, G, end, c) == brute, (first, G, end, c)
                # the shards' tickets are exactly the blocks behind the first G
                assert sum(lib.bshuf_hostcheck_ticket_limit(first, G, end, c) for c in range(S)) == extra
    # fewer blocks than workgroups: no shard owns any
    assert all(lib.bshuf_hostcheck_ticket_limit(0, 10, 4, c) == 0 for c in range(S))


def test_remaining_clamps_over_drawn_counters(lib):
    assert lib.bshuf_hostcheck_ticket_remaining(5, 0) == 5
    assert lib.bshuf_hostcheck_ticket_remaining(5, 4) == 1
    assert lib.bshuf_hostcheck_ticket_remaining(5, 5) == 0
    assert lib.bshuf_hostcheck_ticket_remaining(5, 50000) == 0
    assert lib.bshuf_hostcheck_ticket_remaining(0, 0) == 0
    assert lib.bshuf_hostcheck_ticket_remaining(0, 0xFFFFFFFF) == 0
    assert lib.bshuf_hostcheck_ticket_remaining(1 << 28, 3) == (1 << 28) - 3


def test_victim_choice_on_every_small_vector(lib, S):
    for rem in itertools.product(range(3), repeat=S):
        most = max(rem)
        for own in range(S):
            v = victim(lib, S, rem, own)
            if most == 0:
                assert v == -1
                continue
            assert rem[v] == most
            # the tie goes to the nearest shard behind own, own itself last
            dist = (v - own - 1) % S
            assert all(rem[(own + 1 + d) % S] < most for d in range(dist))


def test_victim_choice_large_values(lib, S):
    rem = [0] * S
    rem[5] = 0xFFFFFFFF
    rem[2] = 0xFFFFFFFE
    assert victim(lib, S, rem, 5) == 5
    assert victim(lib, S, rem, 0) == 5


class Launch:
    """One launch's counters and W waves of the scheme; depth = tickets a wave
    has requested ahead (1: the encoder, 3: the decoder's tk0 for two + tk)."""

    def __init__(self, lib, S, first, W, end, cost, depth, rng, steal=True):
        self.lib, self.S, self.first, self.G, self.end = lib, S, first, W, end
        self.cost, self.depth, self.rng, self.steal = cost, depth, rng, steal
        self.ctr = [0] * S
        self.taken = {}
        self.failed = [0] * W
        self.dropped_valid = 0
        self.stolen = 0

    def block_of(self, shard, t):
        return self.first + self.G + self.S * t + shard

    def limit(self, c):
        return self.lib.bshuf_hostcheck_ticket_limit(self.first, self.G, self.end, c)

    def wave(self, w):
        """Generator: yields the delay to its next step; one shared-memory
        operation (request, peek, draw) happens per step."""
        st = {"shard": w % self.S}
        lat = lambda: float(self.rng.uniform(0.01, 0.3))  # noqa: E731

        def request(n=1):
            t = self.ctr[st["shard"]]
            self.ctr[st["shard"]] += n
            return [(st["shard"], t + k) for k in range(n)]

        def take(ticket):
            shard, t = ticket
            if shard == st["shard"]:
                b = self.block_of(shard, t)
                if b < self.end or not self.steal:
                    return b
            elif self.block_of(shard, t) < self.end:
                self.dropped_valid += 1  # a valid ticket of an abandoned shard: must not happen
            for _ in range(self.S):
                yield lat()
                rem = [self.lib.bshuf_hostcheck_ticket_remaining(self.limit(c), self.ctr[c])
                       for c in range(self.S)]  # peek
                v = victim(self.lib, self.S, rem, st["shard"])
                if v < 0:
                    break
                yield lat()
                t = self.ctr[v]  # draw, waited for
                self.ctr[v] += 1
                b = self.block_of(v, t)
                if b < self.end:
                    if v != w % self.S:
                        self.stolen += 1
                    st["shard"] = v
                    return b
                self.failed[w] += 1
            return self.end

        def do_block(b):
            assert self.first <= b < self.end
            self.taken[b] = self.taken.get(b, 0) + 1

        if self.first + w >= self.end:
            return
        pending = request(self.depth - 1) + request() if self.depth > 1 else request()
        queue = [self.first + w]
        ended = False
        for _ in range(self.depth - 1):  # the decoder's next and nn, before any new request
            if ended:
                break
            b = yield from take(pending.pop(0))
            if b < self.end:
                queue.append(b)
            else:
                ended = True
        while queue:
            blk = queue.pop(0)
            if not ended:
                b = yield from take(pending.pop(0))
                if b < self.end:
                    queue.append(b)
                    pending += request()
                else:
                    ended = True
            do_block(blk)
            yield float(self.cost(blk))
        # whatever is still pending names no block
        for shard, t in pending:
            if self.block_of(shard, t) < self.end:
                self.dropped_valid += 1

    def run(self):
        heap, waves = [], {}
        for w in range(self.G):
            waves[w] = self.wave(w)
            heapq.heappush(heap, (float(self.rng.uniform(0, 0.5)), w))
        steps, done = 0, 0
        budget = 50 * (self.end - self.first + self.G) + 1000
        while heap:
            t, w = heapq.heappop(heap)
            try:
                dt = next(waves[w])
                heapq.heappush(heap, (t + dt, w))
            except StopIteration:
                done += 1
            steps += 1
            assert steps < budget, "a wave does not end"
        assert done == self.G
        return t


def check(L):
    makespan = L.run()
    assert sorted(L.taken) == list(range(L.first, L.end)), "a block was skipped"
    assert set(L.taken.values()) == {1}, "a block was taken twice"
    assert max(L.failed) <= L.S
    assert L.dropped_valid == 0
    return makespan


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("W,extra", [(1, 0), (3, 5), (8, 1), (8, 7), (16, 3), (16, 40), (24, 200), (64, 1000)])
def test_simulation_random_block_times(lib, S, depth, W, extra):
    for seed in range(4):
        rng = np.random.default_rng(1000 * W + 10 * extra + seed)
        first = int(rng.integers(0, 50))
        times = rng.exponential(1.0, W + extra) + 0.05
        check(Launch(lib, S, first, W, first + W + extra, lambda b, f=first, t=times: t[b - f], depth, rng))


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("slow", [0, 3, 7])
def test_simulation_one_shard_50x(lib, S, depth, slow):
    """One shard's blocks cost 50x the others': its tickets must end up with
    the other shards' waves, and the launch must end well before the slow
    shard's own waves could have worked through them."""
    W, extra, first = 32, 1200, 7
    end = first + W + extra

    def cost(b):
        return 50.0 if (b - first - W) % S == slow and b >= first + W else 1.0

    rng = np.random.default_rng(slow)
    stealing = Launch(lib, S, first, W, end, cost, depth, rng)
    t_steal = check(stealing)
    assert stealing.stolen > 0
    rng = np.random.default_rng(slow)
    alone = Launch(lib, S, first, W, end, cost, depth, rng, steal=False)
    t_alone = check(alone)
    assert alone.stolen == 0 and max(alone.failed) == 0
    # 150 slow blocks over 4 waves against over 32: several times shorter
    assert t_steal < 0.5 * t_alone


def test_simulation_counter_headroom(lib, S):
    """Over-draw per wave: its pipeline depth plus at most kTicketShards failed steals."""
    rng = np.random.default_rng(5)
    W, extra = 64, 300
    L = Launch(lib, S, 0, W, W + extra, lambda b: 1.0, 3, rng)
    check(L)
    assert sum(L.ctr) <= extra + W * (3 + S)
